"""Generate tests/golden/ckpt/reference_loads_<Trainer>.npz: what the EXECUTED reference's Load_Mod makes of checkpoints a
PLUGIN trainer wrote (test B of tests/test_checkpoint_interchange.py).

TEST INFRASTRUCTURE (build container only: needs the reference checkout).  For each of DQN_Trainer, DDQN_Trainer,
DuelingDQN_Trainer and SAC_Trainer:

  1. the plugin trainer writes its checkpoints exactly as the test does (tests/test_checkpoint_interchange.py:
     write_plugin_checkpoints -- seeded weights, a few updates, save());
  2. oracle/ref_load_checkpoint.py, in its own process, has a fresh reference trainer's Load_Mod read them and dumps what it
     ended up with: weights, epoch, optimizer moments;
  3. that dump is stored together with the files' contents as torch.load() reads them (flatten_checkpoints, "file|..." keys).

The test then needs no reference: the plugin must still write exactly the recorded contents, and the recorded load must equal
the plugin's own state.

    python oracle/gen_golden_reference_loads.py
"""
from __future__ import annotations

import os
import subprocess
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.abspath(os.path.join(HERE, ".."))
TESTS = os.path.join(ROOT, "tests")
OUT = os.path.join(TESTS, "golden", "ckpt")
for p in (ROOT, TESTS):
    if p not in sys.path:
        sys.path.insert(0, p)
from test_checkpoint_interchange import flatten_checkpoints, write_plugin_checkpoints  # noqa: E402

TRAINERS = ("DQN_Trainer", "DDQN_Trainer", "DuelingDQN_Trainer", "SAC_Trainer")


def main():
    for trainer in TRAINERS:
        with tempfile.TemporaryDirectory() as tmp:
            d = os.path.join(tmp, "Mod")
            write_plugin_checkpoints(trainer, d)
            dump = os.path.join(tmp, "ref_loaded.npz")
            subprocess.run([sys.executable, os.path.join(HERE, "ref_load_checkpoint.py"), trainer, d, dump], check=True, timeout=300)
            with np.load(dump) as z:
                out = {k: z[k] for k in z.files}
            out.update(flatten_checkpoints(d))
        path = os.path.join(OUT, f"reference_loads_{trainer}.npz")
        np.savez_compressed(path, **out)
        print(path, len(out), "arrays")


if __name__ == "__main__":
    main()
