"""Build oracle/_ref/: the reference's own Python modules, byte-compiled (sourceless .pyc, one per module, in the
reference's directory layout), for the CPU test that drives the plugins through the UNMODIFIED reference simulator
(tests/test_plugins.py::test_unmodified_reference_simulator_drives_our_plugins).

TEST INFRASTRUCTURE.  Called by __graft_entry__.build(); needs the reference checkout (ref_harness.REFERENCE_ROOT) and does
nothing without it -- an oracle/_ref/ built earlier is then left as it is.  oracle/_ref/ is a build product: it stays out of
git.  Left out, as in the test: the packages the plugins replace (Envs, Agents, Obstacles, Trainer), checkpoints (Mod) and
the documentation; the config files are written by the test itself (driver.make_config_dir).

    python oracle/build_ref.py
"""
from __future__ import annotations

import os
import py_compile
import shutil
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
OUT = os.path.join(HERE, "_ref")
SKIP_DIRS = {"doc", "Mod", "Envs", "Agents", "Obstacles", "Trainer", "config", ".git"}


def build(out: str = OUT) -> str | None:
    """Byte-compile the reference into `out`; returns `out`, or None when the reference checkout is not there."""
    from oracle.ref_harness import REFERENCE_ROOT
    if not os.path.isdir(REFERENCE_ROOT):
        return None
    tmp = out + ".tmp"
    shutil.rmtree(tmp, ignore_errors=True)
    for d, dirs, files in os.walk(REFERENCE_ROOT):
        dirs[:] = sorted(x for x in dirs if x not in SKIP_DIRS)
        rel = os.path.relpath(d, REFERENCE_ROOT)
        for f in sorted(files):
            if f.endswith(".py"):
                dst = os.path.join(tmp, rel, f[:-3] + ".pyc")
                py_compile.compile(os.path.join(d, f), cfile=dst, dfile=os.path.join(rel, f), doraise=True)
    if not os.path.isfile(os.path.join(tmp, "simulator.pyc")):        # (a checkout this user cannot read)
        shutil.rmtree(tmp, ignore_errors=True)
        return None
    shutil.rmtree(out, ignore_errors=True)
    os.replace(tmp, out)
    return out


if __name__ == "__main__":
    sys.path.insert(0, os.path.dirname(HERE))
    print(build())
