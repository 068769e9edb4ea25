"""The SAC acting launch -- k_sac_act (csrc/sac.hip) through uavenv_sac_act_multi and uavenv_sac_act, and in its place inside
uavenv_sac_loop_run -- held against the float64 forward of oracle/sac_grad_ref.py at every slot count and tile trip, through the C
ABI, on observation rows a real packed ring produced (1 024 envs x 2 UAVs, wrapped; gathered with replacement).

The bar is oracle.sac_grad_ref.act_bar with tau_td = 2^-16 and u = 2^-24: the bar of (h) in tests/test_sac_grad_kernels_gpu.py
(test_act_on_the_stress_actor), where its derivation stands.  Nothing here is wider.

The launch rule (oracle.sac_grad_ref.act_launch_map, asserted for every case before any launch and on the CPU by
tests/test_sac_act_cases.py): max(1, 512 / n) workgroups per slot, tile t of a slot to workgroup t mod gx on trip t div gx.

   n   count                 trips  what it reaches
   1   1, 63, 65               1    edges of a tile
   1   32 768 + 64 + 37        2    workgroups 0 and 1 take a second tile, the last is ragged (37 rows)
   2   333                     1
   3   170 * 64 + 1            2    170 workgroups per slot; workgroup 0's second tile holds one row
   4   8 192 + 333             2    BASELINE configs[3]'s slot count; six workgroups take a second tile, the last has 13 rows
   5   65                      1
   8   2 * 4 096 + 64 + 5      3    workgroups 0 and 1 issue a prefetch from a middle trip (the pipeline's steady state)
Every case in three row layouts: the loop's (first_rows[j] = 37 + j, stride n), blocked (j * count, stride 1), gapped (5 + j,
stride n + 3).  Slot j has its own actor -- fresh and stress actors alternating (stress: oracle.sac_grad_ref.stress_actor tuned
on the slot's own rows; assert_stress on the host for every stress slot of more than 1 000 rows) -- and its own draws.

Per case and layout:
 (a) both planes against actor_forward in f64 within act_bar; everything finite.
 (b) bit for bit what n single uavenv_sac_act launches give on the same inputs (for n >= 2 those take one trip where the batched
     launch takes several).
 (c) planes pre-filled with a sentinel: every row no slot addresses is untouched (gaps, rows past count, 64 rows behind each plane).
 (d) eps = 0: tanh(fc_mu) within the bar; action_bound = 2.5: float32(value at bound 1 * float32(2.5)) bit for bit.
 (e) host only, before the launch, once per case: the f64 side with one thing wrong at a time must be MORE than the two bars apart
     from the right one somewhere (|mutant - right| / (bar(right) + bar(mutant)) > 1: no output can then meet both) -- slot j on
     slot j + 1's draws; the two draw components swapped; slot j with slot j + 1's actor; every slot on slot 0's rows; rows of
     the tiles of trip >= 2 from one trip earlier (i - 64 gx); their draws from one trip earlier; the last row clamped one short
     (count - 2).  Slot mutants need n >= 2, trip mutants a second trip, the clamp count >= 2.
 (f) refusals (test_refusals): UAVENV_EINVAL, uavenv_sac_last_error() set, both planes untouched.
test_wgs_knob_in_a_fresh_child: UAVENV_SAC_ACT_WGS = 8 and 3 (n = 4, count = 333: three and six trips per workgroup; n = 8,
count = 65: two) -- (a) in the child, its planes bit for bit the parent's default-grid planes on the same inputs (hashed).
test_in_the_loop: SACHotLoop(is_train=False), three passes, 8 192 + 64 + 9 envs x 4 UAVs (two trips) and 16 384 + 64 + 9 envs x 2
UAVs (two trips): ring.action[t] and act1_plane[t] bit for bit FusedSACLearner.act_rows per slot on uavenv_randn's draws (a
single-slot, one-trip launch), and both within (a).

MEASURED on an MI355X (printed with -s; the module takes 8 s, the two knob tests 2.4 s each, no other test above 0.6 s).
Worst error / bar:
  (a) 0.1523 over all cases and layouts -- by trips: one 0.1072, two 0.1523, three 0.1523; the three layouts of a case agree to
      the last digit printed; stress actors 0.1523, fresh actors 0.0084; n = 1, count = 32 869 (two trips, one slot): 0.1295
  (d) mean mode 0.1321; action_bound = 2.5: bit for bit everywhere
  (b), (c), (f), the knob's children (their own (a): 0.1095) and the loop (4 UAVs 0.1155, 2 UAVs 0.1176): no bit differed, no
  sentinel was written.  No defect was found: k_sac_act is as it was.
Mutants (e), |mutant - right| / (bar(right) + bar(mutant)), smallest over the cases each applies to (> 1 = told apart):
  next slot's draws 700 889   draws swapped 6 054 (n = 1, count = 1: one row)   next slot's actor 43 343   slot 0's rows 952
  rows one trip back 414 (n = 3: three rows on the second trip)   draws one trip back 3 180   clamp one short 74 (n = 1, count = 63)
"""
import ctypes as C
import hashlib
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from oracle.sac_grad_ref import (PA, act_bar, act_launch_map, actor_forward, actor_head_f64, assert_stress, stress_actor)

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TAU_TD, U = 2.0 ** -16, 2.0 ** -24
SENT = 7.0                      # no action: |action| <= action_bound <= 2.5
CANARY = 64
BASE = 37
LAYOUTS = ("loop", "blocked", "gapped")
# n, count, trips, rows of the last tile, workgroups on the last trip, which slots are stress actors ((j + s0) odd)
CASES = [
    (1, 1, 1, 1, 1, 0), (1, 63, 1, 63, 1, 1), (1, 65, 1, 1, 2, 0),
    (1, 32768 + 64 + 37, 2, 37, 2, 1),
    (2, 333, 1, 13, 6, 1),
    (3, 170 * 64 + 1, 2, 1, 1, 0),
    (4, 8192 + 333, 2, 13, 6, 1),
    (5, 65, 1, 1, 2, 0),
    (8, 2 * 4096 + 64 + 5, 3, 5, 2, 1),
]
KNOB_CASES = [(4, 333, 1), (8, 65, 0)]
WORST, MUT = {}, {}


def check_case_table():
    """What the table claims, from the launch rule alone (no GPU)."""
    for n, count, trips, last, late, _ in CASES:
        m = act_launch_map(n, count)
        assert m["gx"] == max(1, 512 // n) and (m["trips"], m["last"], m["late"]) == (trips, last, late), (n, count, m)
        assert np.array_equal(m["wg"][m["trip"] == trips - 1], np.arange(late))          # the late tiles go to workgroups 0 ..
    m = act_launch_map(1, 32768 + 64 + 37)
    assert m["tiles"] == 514 and list(m["wg"][512:]) == [0, 1] and list(m["trip"][512:]) == [1, 1]
    m = act_launch_map(3, 170 * 64 + 1)
    assert m["gx"] == 170 and m["tiles"] == 171 and m["wg"][170] == 0 and m["last"] == 1
    m = act_launch_map(4, 8192 + 333)
    assert m["gx"] == 128 and m["tiles"] == 134
    m = act_launch_map(8, 2 * 4096 + 64 + 5)
    assert m["gx"] == 64 and m["tiles"] == 130 and list(m["trip"][[0, 64, 128]]) == [0, 1, 2] and list(m["wg"][[0, 64, 128]]) == [0, 0, 0]
    assert list(m["trip"][[1, 65, 129]]) == [0, 1, 2] and m["trip"][127] == 1 and m["wg"][127] == 63       # the rest: two trips
    # the knob's children
    assert [act_launch_map(4, 333, b)[k] for b in (8, 3) for k in ("gx", "trips")] == [2, 3, 1, 6]
    assert [act_launch_map(8, 65, b)[k] for b in (8, 3) for k in ("gx", "trips")] == [1, 2, 1, 2]
    # the loop test's envs
    assert act_launch_map(4, 8192 + 64 + 9)["trips"] == 2 and act_launch_map(2, 16384 + 64 + 9)["trips"] == 2
    assert act_launch_map(1, 8192 + 64 + 9)["trips"] == 1 and act_launch_map(1, 16384 + 64 + 9)["trips"] == 1


def _lib():
    from dqn_based_uav_3d_path_planer_amd import _lib as L
    return L


def stream():
    return torch.cuda.current_stream().cuda_stream


def note(key, v, book=WORST, pick=max):
    book[key] = pick(book.get(key, v), float(v))


_POOL = None
_FRESH = None


def pool():
    global _POOL
    if _POOL is None:
        from test_sac_grad_kernels_gpu import Pool
        _POOL = Pool()
    return _POOL


def param():
    from test_sac_grad_kernels_gpu import PARAM
    return PARAM


def fresh_flats():
    """Eight freshly initialised actors (flat blocks, float32 [PA])."""
    global _FRESH
    if _FRESH is None:
        from dqn_based_uav_3d_path_planer_amd.sac import FusedSACLearner
        _FRESH = []
        for j in range(8):
            torch.manual_seed(100 + j)
            _FRESH.append(FusedSACLearner(param())._blocks[0, :PA].cpu().numpy().copy())
    return _FRESH


@pytest.fixture(scope="module", autouse=True)
def _release_pool():
    global _POOL
    yield
    print("SAC acting, worst error / bar:", {k: round(v, 4) for k, v in sorted(WORST.items())})
    print("SAC acting, mutants, smallest |mutant - right| / (two bars) over the cases:", {k: round(v, 2) for k, v in sorted(MUT.items())})
    if _POOL is not None:
        _POOL.env.close()
        _POOL = None
        torch.cuda.synchronize()
        torch.cuda.empty_cache()


def slim(hd):
    for k in ("pre", "H", "habs"):
        hd.pop(k, None)
    return hd


def rehead(hd, idx, eps):
    """The head of hd's rows `idx` on the draws eps: what act_bar and the comparison need."""
    o = hd["o"][idx]
    d = actor_head_f64(o[:, :2], o[:, 2:], eps)
    d.update(m_abs=hd["m_abs"][idx], s_abs=hd["s_abs"][idx], eps=np.asarray(eps, dtype=np.float64))
    return d


class Inputs:
    """One case's host side: per slot the pool rows it reads (gathered with replacement), its actor, its draws, and the f64 forward."""

    def __init__(self, n, count, s0, seed=0, rows=None, flats=None):
        """rows / flats: the observation rows to gather from and the fresh actors (default: the pool's, fresh_flats()) -- host only
        until upload()."""
        rows = pool().rows if rows is None else rows
        rng = np.random.default_rng([seed, n, count])
        self.n, self.count, self.rng = n, count, rng
        self.src = rng.integers(0, len(rows), (n, count))
        self.X = [rows[self.src[j]] for j in range(n)]
        self.eps = rng.normal(size=(n, count, 2)).astype(np.float32)
        self.kinds = ["stress" if (j + s0) % 2 else "fresh" for j in range(n)]
        self.flat = []
        for j, f in enumerate((fresh_flats() if flats is None else flats)[:n]):
            if self.kinds[j] == "stress":            # tuned on the slot's own rows (one row alone spans nothing: the pool's then)
                f = stress_actor(f, self.X[j] if count > 1 else rows).astype(np.float32)
            self.flat.append(f)
        self.hd = [slim(actor_forward(self.X[j], self.flat[j], self.eps[j])) for j in range(n)]
        self.hd_mean = [slim(actor_forward(self.X[j], self.flat[j], np.zeros((count, 2)))) for j in range(n)]
        for j in range(n):
            if self.kinds[j] == "stress" and count > 1000:
                assert_stress(self.hd[j])

    def upload(self):
        self.actors = [torch.tensor(f).cuda().contiguous() for f in self.flat]
        self.eps_dev = [torch.tensor(self.eps[j]).cuda().contiguous() for j in range(self.n)]
        self.zero = torch.zeros((self.count, 2), device="cuda")
        return self

    def mutants(self):
        """(e) -> {name: worst |mutant - right| / (bar(right) + bar(mutant))} for the mutants that apply to this case."""
        n, count = self.n, self.count
        m = act_launch_map(n, count)
        i = np.arange(count)
        late = m["trip"][i // 64] >= 1
        back = np.where(late, i - 64 * m["gx"], i)
        assert back.min() >= 0 and (late.any() == (m["trips"] > 1))
        out = {}

        def add(name, j, d):
            r = np.abs(d["act"] - self.hd[j]["act"]) / (act_bar(self.hd[j], TAU_TD, U) + act_bar(d, TAU_TD, U))
            out[name] = max(out.get(name, 0.0), float(r.max()))
        for j in range(n):
            hd, nx = self.hd[j], (j + 1) % n
            add("draws swapped", j, rehead(hd, i, self.eps[j][:, ::-1]))
            if n >= 2:
                add("next slot's draws", j, rehead(hd, i, self.eps[nx]))
                add("next slot's actor", j, slim(actor_forward(self.X[j], self.flat[nx], self.eps[j])))
                if j:
                    add("slot 0's rows", j, slim(actor_forward(self.X[0], self.flat[j], self.eps[j])))
            if m["trips"] > 1:
                add("rows one trip back", j, rehead(hd, back, self.eps[j]))
                add("draws one trip back", j, rehead(hd, i, self.eps[j][back]))
            if count >= 2:
                add("clamp one short", j, rehead(hd, np.minimum(i, count - 2), self.eps[j]))
        return out


class Layout:
    def __init__(self, kind, inp):
        n, count = inp.n, inp.count
        if kind == "loop":
            self.first, self.stride = [BASE + j for j in range(n)], n
        elif kind == "blocked":
            self.first, self.stride = [j * count for j in range(n)], 1
        else:
            self.first, self.stride = [5 + j for j in range(n)], n + 3
        self.rows = [f + self.stride * np.arange(count) for f in self.first]
        self.total = int(max(r[-1] for r in self.rows)) + 1
        self.mask = np.zeros(self.total + CANARY, dtype=bool)
        for r in self.rows:
            assert not self.mask[r].any()                                # no two slots share a row
            self.mask[r] = True
        p = pool()
        fill = inp.rng.integers(0, len(p.rows), self.total)              # rows nobody addresses hold other observations
        for j, r in enumerate(self.rows):
            fill[r] = inp.src[j]
        self.obs = p.packed[torch.tensor(fill, device="cuda")].contiguous()
        assert self.obs.shape[0] == self.total and self.obs.data_ptr() % 16 == 0


def launch(inp, lay, eps, bound=1.0, single=False, obs_ptr=None):
    """-> (rc of the launch(es), act0, act1 as numpy [total + CANARY]); eps: one device tensor per slot."""
    lib = _lib().load()
    n = inp.n
    a0 = torch.full((lay.total + CANARY,), SENT, device="cuda")
    a1 = torch.full((lay.total + CANARY,), SENT, device="cuda")
    assert all(e.numel() == 2 * inp.count for e in eps) and max(int(r[-1]) for r in lay.rows) < lay.total
    obs = lay.obs.data_ptr() if obs_ptr is None else obs_ptr
    if single:
        rc = 0
        for j in range(n):
            rc = rc or lib.uavenv_sac_act(inp.actors[j].data_ptr(), obs, lay.first[j], lay.stride, inp.count, eps[j].data_ptr(), bound,
                                          a0.data_ptr(), a1.data_ptr(), stream())
    else:
        actors = (C.c_void_p * n)(*[a.data_ptr() for a in inp.actors])
        first = (C.c_int32 * n)(*lay.first)
        epss = (C.c_void_p * n)(*[e.data_ptr() for e in eps])
        rc = lib.uavenv_sac_act_multi(C.addressof(actors), obs, C.addressof(first), lay.stride, inp.count, C.addressof(epss), bound,
                                      a0.data_ptr(), a1.data_ptr(), n, stream())
    torch.cuda.synchronize()
    assert rc == 0, (rc, lib.uavenv_sac_last_error())
    return a0.cpu().numpy(), a1.cpu().numpy()


def bits(x):
    return np.ascontiguousarray(x, dtype=np.float32).view(np.uint32)


def untouched(lay, p0, p1):
    s = bits(np.float32(SENT))
    return bool((bits(p0)[~lay.mask] == s).all() and (bits(p1)[~lay.mask] == s).all())


def ratio_a(lay, p0, p1, hds, kinds=None):
    """(a): worst |plane - act| / act_bar over the slots' rows; asserts finiteness."""
    worst = 0.0
    for j, (r, hd) in enumerate(zip(lay.rows, hds)):
        got = np.stack([p0[r], p1[r]], 1).astype(np.float64)
        assert np.isfinite(got).all()
        w = float((np.abs(got - hd["act"]) / act_bar(hd, TAU_TD, U)).max())
        if kinds is not None:
            note("(a) %s actors" % kinds[j], w)
        worst = max(worst, w)
    return worst


def run_case(n, count, s0, layouts=LAYOUTS, tag="", seed=0, with_mutants=True):
    """-> (the case's Inputs, {layout: (act0, act1, Layout)} of the batched launch on the case's own draws)."""
    inp = Inputs(n, count, s0, seed)
    m = act_launch_map(n, count)
    key = "n=%d count=%d%s" % (n, count, tag)
    if with_mutants:                                    # (e), before any launch
        res = inp.mutants()
        print(key, "trips", m["trips"], "mutants:", {k: round(v, 2) for k, v in res.items()})
        want = {"draws swapped"} | ({"next slot's draws", "next slot's actor", "slot 0's rows"} if n >= 2 else set()) | \
            ({"rows one trip back", "draws one trip back"} if m["trips"] > 1 else set()) | ({"clamp one short"} if count >= 2 else set())
        assert set(res) == want
        for k, v in res.items():
            note(k, v, MUT, min)
            assert v > 1.0, (key, "the inputs cannot tell this mutant from the original", k, v)
    inp.upload()
    planes = {}
    for kind in layouts:
        lay = Layout(kind, inp)
        p0, p1 = launch(inp, lay, inp.eps_dev)
        ra = ratio_a(lay, p0, p1, inp.hd, inp.kinds)                                        # (a)
        s0_, s1_ = launch(inp, lay, inp.eps_dev, single=True)                               # (b)
        same = np.array_equal(bits(p0), bits(s0_)) and np.array_equal(bits(p1), bits(s1_))
        clean = untouched(lay, p0, p1)                                                      # (c)
        z0, z1 = launch(inp, lay, [inp.zero] * n)                                           # (d)
        rm = ratio_a(lay, z0, z1, inp.hd_mean)
        b0, b1 = launch(inp, lay, inp.eps_dev, bound=2.5)
        scaled = all(np.array_equal(bits(b[lay.mask]), bits(p[lay.mask] * np.float32(2.5))) for b, p in ((b0, p0), (b1, p1)))
        print(key, kind, "(a) %.4f  mean mode %.4f  single launches equal: %s" % (ra, rm, same))
        note("(a)" + tag, ra)
        note("(a) %d trip(s)%s" % (m["trips"], tag), ra)
        note("(d) mean mode" + tag, rm)
        assert ra <= 1.0, (key, kind, "(a)", ra)
        assert same, (key, kind, "(b) the batched launch differs from n single launches")
        assert clean and untouched(lay, z0, z1) and untouched(lay, b0, b1), (key, kind, "(c) a row no slot addresses was written")
        assert rm <= 1.0, (key, kind, "(d) mean mode", rm)
        assert scaled, (key, kind, "(d) action_bound = 2.5")
        planes[kind] = (p0, p1, lay)
    return inp, planes


def test_the_case_table_is_what_the_launch_rule_gives():
    check_case_table()


@pytest.mark.parametrize("case", CASES, ids=lambda c: "n%d-%d" % (c[0], c[1]))
def test_act_multi_against_f64(case):
    check_case_table()
    n, count, _, _, _, s0 = case
    run_case(n, count, s0)


def test_refusals():
    """(f)"""
    L = _lib()
    lib = L.load()
    inp = Inputs(2, 65, 1).upload()
    lay = Layout("loop", inp)
    n = inp.n
    a0 = torch.full((lay.total + CANARY,), SENT, device="cuda")
    a1 = torch.full((lay.total + CANARY,), SENT, device="cuda")
    good = dict(actors=[a.data_ptr() for a in inp.actors], obs=lay.obs.data_ptr(), first=list(lay.first), stride=lay.stride,
                count=inp.count, eps=[e.data_ptr() for e in inp.eps_dev], a0=a0.data_ptr(), a1=a1.data_ptr(), n=n)

    def call(**kw):
        a = dict(good, **kw)
        k = len(a["actors"])
        assert k >= a["n"] and len(a["first"]) == k and len(a["eps"]) == k
        actors = (C.c_void_p * k)(*a["actors"])
        first = (C.c_int32 * k)(*a["first"])
        epss = (C.c_void_p * k)(*a["eps"])
        return lib.uavenv_sac_act_multi(C.addressof(actors), a["obs"], C.addressof(first), a["stride"], a["count"], C.addressof(epss), 1.0,
                                        a["a0"], a["a1"], a["n"], stream())
    nine = [j % 2 for j in range(9)]                     # nine used slots, every one of them valid on its own
    bad = {"n = 0": dict(n=0), "n = 9": dict(n=9, actors=[good["actors"][j] for j in nine], first=[lay.first[j] for j in nine],
                                              eps=[good["eps"][j] for j in nine]),
           "count = 0": dict(count=0), "row_stride = 0": dict(stride=0),
           "null actor": dict(actors=[good["actors"][0], None]), "null eps": dict(eps=[None, good["eps"][1]]),
           "negative first row": dict(first=[lay.first[0], -1]),
           "obs off alignment": dict(obs=good["obs"] + 4), "actor off alignment": dict(actors=[good["actors"][0] + 4, good["actors"][1]]),
           "null act0": dict(a0=None), "null act1": dict(a1=None)}
    for what, kw in bad.items():
        # another entry point's refusal first, so that the message read below is this call's
        assert lib.uavenv_sac_actor_adam(None, None, 0, 0, None, None, None, None, 0.0, 0.0, None, stream()) == L.EINVAL
        assert lib.uavenv_sac_last_error().startswith(b"uavenv_sac_actor_adam")
        rc = call(**kw)
        assert rc == L.EINVAL, (what, rc)
        assert lib.uavenv_sac_last_error().startswith(b"uavenv_sac_act:"), (what, lib.uavenv_sac_last_error())
    assert lib.uavenv_sac_act(None, good["obs"], lay.first[0], lay.stride, inp.count, good["eps"][0], 1.0, good["a0"], good["a1"],
                              stream()) == L.EINVAL
    torch.cuda.synchronize()
    assert bool((a0 == SENT).all()) and bool((a1 == SENT).all())
    assert call() == 0                                   # and the same arguments unspoilt are taken
    torch.cuda.synchronize()
    p0, p1 = a0.cpu().numpy(), a1.cpu().numpy()
    assert ratio_a(lay, p0, p1, inp.hd) <= 1.0 and untouched(lay, p0, p1)


def knob_digest(inp, lay):
    h = hashlib.sha256()
    for t in [lay.obs] + inp.actors + inp.eps_dev:
        h.update(t.cpu().numpy().tobytes())
    return h.hexdigest()


def knob_run(path=None):
    """The knob's cases on seeded inputs in the loop's layout: (a) .. (d) as everywhere; -> (or written to `path`) the planes and a
    digest of the inputs."""
    out = {}
    for k, (n, count, s0) in enumerate(KNOB_CASES):
        inp, planes = run_case(n, count, s0, layouts=("loop",), tag=" knob", seed=7, with_mutants=path is None)
        out["act0_%d" % k], out["act1_%d" % k], lay = planes["loop"]
        out["digest_%d" % k] = np.frombuffer(bytes.fromhex(knob_digest(inp, lay)), dtype=np.uint8)
    if path is not None:
        np.savez(path, **out)
    return out


CHILD = r"""
import sys
sys.path.insert(0, sys.argv[1])
sys.path.insert(0, sys.argv[1] + "/tests")
import torch
torch.cuda.set_device(0)
import test_sac_act_kernels_gpu as T
T.knob_run(sys.argv[2])
print("knob worst ratios", T.WORST)
T.pool().env.close()
"""


@pytest.mark.parametrize("wgs", ["8", "3"])
def test_wgs_knob_in_a_fresh_child(wgs, tmp_path):
    """UAVENV_SAC_ACT_WGS (read once per process: a fresh child under its own time limit).  A row's instructions do not depend on
    its trip: any bit that differs from the default grid's planes is a defect."""
    check_case_table()
    env = {k: v for k, v in os.environ.items() if not k.startswith("UAVENV_")}
    env["UAVENV_SAC_ACT_WGS"] = wgs
    path = str(tmp_path / "planes.npz")
    subprocess.run(["timeout", "-k", "10", "300", sys.executable, "-c", CHILD, ROOT, path], env=env, check=True, timeout=330)
    mine = knob_run()
    with np.load(path) as z:
        theirs = {k: z[k] for k in z.files}
    assert set(theirs) == set(mine)
    for k in sorted(mine):
        if k.startswith("digest"):
            assert np.array_equal(mine[k], theirs[k]), "the child ran on other inputs"
    for k in sorted(mine):
        assert np.array_equal(bits(mine[k]) if k.startswith("act") else mine[k], bits(theirs[k]) if k.startswith("act") else theirs[k]), \
            (wgs, k, "differs from the default grid")


@pytest.mark.parametrize("uav,envs", [(4, 8192 + 64 + 9), (2, 16384 + 64 + 9)])
def test_in_the_loop(uav, envs):
    """k_sac_act where the benchmark runs it: uavenv_sac_loop_run's one launch for all slots (two trips at these sizes) against
    FusedSACLearner.act_rows slot by slot (one trip) on the same frame and uavenv_randn's draws, and against f64."""
    from dqn_based_uav_3d_path_planer_amd.data import make_city26_env
    from dqn_based_uav_3d_path_planer_amd.loop import SACHotLoop
    from dqn_based_uav_3d_path_planer_amd.replay import DeviceReplayRing
    from dqn_based_uav_3d_path_planer_amd.sac import FusedSACLearner
    check_case_table()
    L = _lib()
    lib = L.load()
    tune = pool().rows
    env = make_city26_env(envs, uav_per_env=uav, obs_dtype="packed")
    N = env.N
    assert N == uav * envs
    ring = DeviceReplayRing(env, 3 * N, discrete=False)
    assert ring.frames == 4
    ring.reset(seed=6)
    a1 = torch.full((ring.frames, N), SENT, device="cuda")
    ring.action.fill_(SENT)
    Ls = []
    for j in range(uav):
        torch.manual_seed(300 + j)
        Lj = FusedSACLearner(param())
        if j % 2:
            with torch.no_grad():
                Lj._blocks[0, :PA].copy_(torch.tensor(stress_actor(Lj._blocks[0].cpu().numpy(), tune).astype(np.float32)).cuda())
        Ls.append(Lj)
    flats = [Lj._blocks[0].cpu().numpy().astype(np.float64) for Lj in Ls]
    seed, counter0, batch = (0x5AC << 32) | 1234, 41, 64
    loop = SACHotLoop(ring, Ls, batch, seed=seed, act1_plane=a1, counter=counter0, is_train=False)
    n_noise = int(lib.uavenv_sac_loop_noise_floats(uav, envs, batch))
    flat_obs = ring.obs.view(-1, ring.obs.shape[-1])
    worst, acted = 0.0, []
    for k in range(3):
        t = ring.head
        loop.run(1)
        z = torch.empty(n_noise, device="cuda")
        assert lib.uavenv_randn(seed, counter0 + 1 + k, n_noise, z.data_ptr(), stream()) == 0
        p0 = torch.full((ring.frames * N,), SENT, device="cuda")
        p1 = torch.full((ring.frames * N,), SENT, device="cuda")
        eps = [z[j * 2 * envs:(j + 1) * 2 * envs].view(envs, 2) for j in range(uav)]
        for j in range(uav):
            Ls[j].act_rows(flat_obs, t * N + j, uav, envs, p0, p1, eps[j])
        torch.cuda.synchronize()
        assert torch.equal(loop._noise, z)
        assert torch.equal(ring.action[t].view(torch.int32), p0.view(ring.frames, N)[t].view(torch.int32)), ("act0", k)
        assert torch.equal(a1[t].view(torch.int32), p1.view(ring.frames, N)[t].view(torch.int32)), ("act1", k)
        acted.append(t)
        for other in range(ring.frames):                          # (c) in its place: frames no pass has acted on stay as they were
            if other not in acted:
                assert bool((ring.action[other] == SENT).all()) and bool((a1[other] == SENT).all()), (k, other)
            if other != t:
                assert bool((p0.view(ring.frames, N)[other] == SENT).all()) and bool((p1.view(ring.frames, N)[other] == SENT).all())
        rows = torch.empty((N, 100), dtype=torch.float32, device="cuda")
        assert lib.uavenv_obs_unpack(ring.obs[t].data_ptr(), N, rows.data_ptr(), L.OBS_F32, stream()) == 0
        torch.cuda.synchronize()
        X = rows.cpu().numpy()
        g0, g1 = ring.action[t].cpu().numpy(), a1[t].cpu().numpy()
        for j in range(uav):
            hd = slim(actor_forward(X[j::uav], flats[j], eps[j].cpu().numpy()))
            got = np.stack([g0[j::uav], g1[j::uav]], 1).astype(np.float64)
            assert np.isfinite(got).all()
            worst = max(worst, float((np.abs(got - hd["act"]) / act_bar(hd, TAU_TD, U)).max()))
    note("(a) in the loop, %d UAVs" % uav, worst)
    print("in the loop, %d envs x %d UAVs, three passes: (a) %.4f" % (envs, uav, worst))
    loop.close()
    env.close()
    assert worst <= 1.0, worst
