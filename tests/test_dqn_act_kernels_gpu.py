"""Every DQN acting form -- the eight dispatch targets of uavenv_dqn_act (csrc/learner.hip: k_dqn_act<float | __half, 4 | NMAX>,
k_dqn_act_packed<4 | NMAX>, k_dqn_act_h<PACKED | F16>), uavenv_select_actions (csrc/replay.hip) and the policy prologues of the
step launches (k_step_coop<.., POLICY> with and without the layer-1 image, k_step_polh) -- held against the float64 forward and
the Philox stream of oracle/dqn_act_ref.py, through the C ABI, on observation rows the environment really produces.

 (a) Q against f64, every row and action: |q_out - Q| <= tau_q q_abs, tau_q = 2^-16 (q_abs: the |.|-propagated forward).  The
     derivation is tests/test_dqn_grad_kernels_gpu.py's: layer 1 sums 101 terms, layer 2 65, the dueling combine up to 15 more,
     each rounded once at u = 2^-24: < 256 u.  The f16-MFMA forms are held to the SAME bar against the reference fed the operands
     they round by design (rows, fc1 and b1 to f16: oracle/dqn_act_ref.f16_operands); products of two f16 values are exact in
     f32, the sums are f32, layer 2 is f32 on the unrounded H.
     For n >= 1000, over all (row, action) pairs with e = (q_out - Q) / q_abs: rms(e) <= 2 sig_td and |mean(e)| <= K sig_td /
     sqrt(n A), sig_td = 2^-20, K = 6.  These two are the bars the issue behind this test set, not a strict derivation: the
     errors of different rows are independent round-to-nearest errors of standard deviation <= sig_td q_abs, but the A actions
     of one row share their layer-1 roundings and are correlated, so sqrt(n A) overstates the independent count by up to
     sqrt(A); the measured means stay below 0.08 of the bar, far inside that factor (sqrt(14) = 3.7).
 (b) the decision, no ambiguity window: index_out == decide(q_out) for EVERY row -- the first maximum of the kernel's own Q
     values where float32(u) > float32(eps), the oracle's random action otherwise -- and steer_out == float32(-1 + 2 a / (A - 1))
     bit for bit; eps in {-1, 0, 0.1, 1, u[j]} (u[j]: a draw the oracle names; row j then takes rnd[j] and the row of the next
     larger draw is greedy: the strict >); seed and counter both above 2^32 in every call; index_out alone, steer_out alone and
     q_out null give the same results.  With (a) this pins the action to f64 without skipping a row.
 (c) exact ties (two identical layer-2 rows and biases): the two Q values bit-equal, the lower index wins.
 (d) uavenv_select_actions on hand-built tables (ties, +-inf, all-equal rows; one trip past its grid cap) == decide, and ==
     uavenv_dqn_act on that call's own q_out.
 (e) the in-step policy: the action plane the step launch writes == uavenv_dqn_act's index_out on the same current rows, for
     every agent the step reports valid; that index_out is held by (a) and (b) in the same test.
 (f) mutations of the f64 side (host only, n = 1000): the named check alone must reject each.

Head sizes: A = 3 plain (q_strip's n2 == 3 copy), 3 dueling (n2 == 4 copy), 2, 4 plain, 9 dueling, and net_ok's limits 14 plain
and 13 dueling (general path); fresh nets and the trained nets of the packed learner goldens (|Q| up to 15, q_abs up to 380),
carried to the other head sizes by tests/dqn_fixtures.widen_head.  Row counts 1, 63, 65, 1000; k_dqn_act_h also 512 * 64 + 64
+ 37 = 32 869: some workgroups take a second tile and the last tile is ragged.

MEASURED on an MI355X (printed with -s; the module takes 6 s of wall time, 3 s of it in the tests, no case above 0.5 s).
Worst error / bar per form over all heads, nets and sizes -- (a) hard bar / rms bar / mean bar; (b), (c), (d), (e) are exact
and had no mismatch in any row:
  k_dqn_act<float, 4>   0.0019 / 0.0043 / 0.041     k_dqn_act<float, NMAX>  0.0022 / 0.0041 / 0.059
  k_dqn_act<__half, 4>  0.0019 / 0.0043 / 0.041     k_dqn_act<__half, NMAX> 0.0023 / 0.0041 / 0.062
  k_dqn_act_packed<4>   0.0016 / 0.0030 / 0.012     k_dqn_act_packed<NMAX>  0.0017 / 0.0029 / 0.018
  k_dqn_act_h<F16>      0.0020 / 0.0028 / 0.074     k_dqn_act_h<PACKED>     0.0020 / 0.0028 / 0.075   (n = 32 869 included)
  rows of the step launches (e): k_step_coop's 0.0030 / 0.0045 / 0.011, k_step_polh's 0.0030 (N = 962: no aggregate)
  The f16-MFMA forms meet the f32 bar against the reference fed f16 rows, fc1 and b1: they round nothing else.
  The hard bar is a worst-case bound and ~500 x above the errors seen; the aggregate bars are what resolve small uniform errors.
Mutations, smallest ratio over the forms (> 1 = rejected):
  most often set flag's column zeroed 44.6 | b1 of a live unit dropped 18.0 | one b2 dropped 23.4 | dueling mean over A + 1 19.4  -- (a), hard bar
  last maximum: every row | >= for >: row j | floor(u A): 49 % of rows | counter's low half: 49 % | seed's low half: 52 %  -- (b), (c)
  flag columns of fc1 rounded to f16 (split layer 1 without mid * 2^-11), f32-MFMA packed forms: the hard bar CANNOT see it
  (0.05 .. 0.26) and neither can the rms bar (0.13 .. 0.91).  The mean bar rejects it on every trained net, which is ASSERTED
  for both packed forms: k_dqn_act_packed<4> 1.375 (A = 3 dueling) .. 12.9 (the Qnet2 golden itself: 12.8), k_dqn_act_packed<NMAX>
  2.24 (A = 9 dueling) .. 28.  On the fresh nets it is only recorded: rejected with A = 2, 4, 14 and 3 dueling (1.1 .. 10), NOT
  with A = 3 plain (0.54), 9 dueling (0.27) and 13 dueling (0.86): a freshly initialised net's flag weights are too small for
  any bar here to notice the second term's absence.
  Every output buffer carries 130 sentinel rows behind row n - 1; none was written.
"""
import ctypes as C
import time

import numpy as np
import pytest
import torch

from conftest import load_golden, pack_obs_rows
from dqn_fixtures import Pool, golden_flat, tie_rows, unpack, widen_head
from oracle.dqn_act_ref import FLAG_COLS, act_f64, decide, draws, first_argmax, steer_of
from oracle.dqn_grad_ref import forward_f64, unflatten

pytestmark = pytest.mark.gpu

TAU_Q, SIG_TD, K = 2.0 ** -16, 2.0 ** -20, 6.0
HI = 1 << 32
SMALL = [(3, False), (3, True), (2, False), (4, False)]
LARGE = [(9, True), (14, False), (13, True)]
SIZES = (1, 63, 65, 1000)
N_H2 = 512 * 64 + 64 + 37
# (rows, MFMA): the eight dispatch targets are the three f32-MFMA row kinds x (n2 <= 4, larger) and the two f16-MFMA row kinds
FORMS = [("f32", "f32"), ("f16", "f32"), ("packed", "f32"), ("f16", "f16"), ("packed", "f16")]
CASES = [(r, m, A, d, net) for (r, m) in FORMS for (A, d) in (SMALL + LARGE if m == "f32" else SMALL) for net in ("fresh", "stress")]
WORST, MUT, T0 = {}, {}, time.time()


def _lib():
    from dqn_based_uav_3d_path_planer_amd import _lib as L
    return L


_POOL = None


def pool():
    global _POOL
    if _POOL is None:
        _POOL = Pool()
    return _POOL


@pytest.fixture(scope="module", autouse=True)
def _release_pool():
    """The pool's environment and ring live for this module only: later modules time their own loops on the same device."""
    global _POOL
    yield
    print("module wall time %.1f s" % (time.time() - T0), "worst ratios", {k: round(v, 4) for k, v in sorted(WORST.items())},
          "mutations (smallest rejecting ratio)", {k: round(v, 3) for k, v in sorted(MUT.items())})
    if _POOL is not None:
        _POOL.env.close()
        _POOL = None
        torch.cuda.synchronize()
        torch.cuda.empty_cache()


def fresh_flat(A, dueling, seed):
    from dqn_based_uav_3d_path_planer_amd.nets import create_network
    torch.manual_seed(seed)
    net = create_network({"NetWork": "VAnet2" if dueling else "Qnet2", "w": "100", "hiden_dim": "64", "output": str(A)})
    return golden_flat({k: v.detach().numpy() for k, v in net.state_dict().items()}, "", dueling)


def stress_flat(A, dueling):
    g = load_golden("learner_%s_packed.npz" % ("DuelingDQN_Trainer" if dueling else "DQN_Trainer"))
    return widen_head(golden_flat(g, "l1_", dueling), A, dueling)


class Net:
    """A flat parameter block on the device (local = target; zero moments) and its UavDqnNet."""

    def __init__(self, flat, A, dueling, mfma):
        L = _lib()
        self.flat, self.A, self.dueling, self.mfma = np.asarray(flat, dtype=np.float32), A, dueling, mfma
        P = self.flat.size
        self.buf = torch.zeros((4, (P + 3) & ~3), dtype=torch.float32, device="cuda")     # every block 16-byte aligned
        self.buf[:2, :P] = torch.tensor(self.flat, device="cuda")
        self.net = L.UavDqnNet(self.buf[0].data_ptr(), self.buf[1].data_ptr(), self.buf[2].data_ptr(), self.buf[3].data_ptr(),
                               100, 64, A, 1 if dueling else 0, L.MFMA_F16 if mfma == "f16" else L.MFMA_F32, 0)
        assert L.load().uavenv_dqn_num_params(C.byref(self.net)) == P

    def image(self):
        L = _lib()
        img = torch.empty(2 * L.DQN_IMAGE_FLOATS, dtype=torch.float32, device="cuda")
        assert L.load().uavenv_dqn_split_image(C.byref(self.net), img.data_ptr(), stream()) == 0
        return img


def stream():
    return torch.cuda.current_stream().cuda_stream


def store(rows, kind):
    """rows [n, 100] f32 -> (device tensor as the kernels read it, obs code, the values it holds as f64)."""
    L = _lib()
    if kind == "packed":
        return torch.tensor(pack_obs_rows(rows), device="cuda").contiguous(), L.OBS_PACKED, rows.astype(np.float64)
    if kind == "f16":
        h = rows.astype(np.float16)
        return torch.tensor(h, device="cuda").contiguous(), L.OBS_F16, h.astype(np.float64)
    return torch.tensor(rows, device="cuda").contiguous(), L.OBS_F32, rows.astype(np.float64)


def act(net, obs, code, n, eps, seed, counter, want="isq", expect=0):
    """uavenv_dqn_act into sentinel-filled outputs -> (index, steer bits, q) of rows 0 .. n - 1 as numpy (None where not asked
    for).  Every output has GUARD more rows behind row n - 1, which must come back untouched: a ragged last tile or a second
    trip round a persistent loop must not write past n."""
    idx, st, q = out_bufs(n, net.A, want)
    p = lambda t: None if t is None else t.data_ptr()  # noqa: E731
    rc = _lib().load().uavenv_dqn_act(C.byref(net.net), obs.data_ptr(), code, n, float(eps), seed, counter, p(idx), p(st), p(q),
                                      stream())
    assert rc == expect, rc
    torch.cuda.synchronize()
    return read_bufs(n, idx, st, q)


GUARD = 130          # rows behind the last one: more than the two 64-row tiles a stray workgroup could add


def out_bufs(n, A, want="isq"):
    idx = torch.full((n + GUARD,), -7, dtype=torch.int32, device="cuda") if "i" in want else None
    st = torch.full((n + GUARD,), float("nan"), device="cuda") if "s" in want else None
    q = torch.full((n + GUARD, A), float("nan"), device="cuda") if "q" in want else None
    return idx, st, q


def read_bufs(n, idx, st, q):
    c = lambda t: None if t is None else t.cpu().numpy()  # noqa: E731
    idx, st, q = c(idx), c(st), c(q)
    assert idx is None or np.all(idx[n:] == -7), "index_out written past n"
    assert st is None or np.isnan(st[n:]).all(), "steer_out written past n"
    assert q is None or np.isnan(q[n:]).all(), "q_out written past n"
    return (None if idx is None else idx[:n], None if st is None else st[:n].view(np.uint32), None if q is None else q[:n])


def ratios(q_out, Q, q_abs):
    """(hard, rms, mean): the worst |e| / tau_q, rms(e) / (2 sig_td), |mean(e)| / (K sig_td / sqrt(n A)); e = (q_out - Q) / q_abs."""
    e = (q_out.astype(np.float64) - Q) / q_abs
    return (float(np.abs(e).max() / TAU_Q), float(np.sqrt(np.mean(e * e)) / (2 * SIG_TD)),
            float(abs(e.mean()) / (K * SIG_TD / np.sqrt(e.size))))


def check_a(key, q_out, Q, q_abs, say=True):
    assert np.isfinite(q_out).all()
    hard, rms, mean = ratios(q_out, Q, q_abs)
    WORST[key + " a"] = max(WORST.get(key + " a", 0.0), hard)
    if len(Q) >= 1000:
        WORST[key + " rms"] = max(WORST.get(key + " rms", 0.0), rms)
        WORST[key + " mean"] = max(WORST.get(key + " mean", 0.0), mean)
        if say:
            print(key, "n", len(Q), "hard %.4f rms %.4f mean %.4f" % (hard, rms, mean))
        assert rms <= 1.0 and mean <= 1.0, (key, rms, mean)
    assert hard <= 1.0, (key, hard)


def check_b(idx, steer_bits, q_out, u, rnd, eps, A):
    want = decide(q_out, u, rnd, eps)
    assert np.array_equal(idx, want), (eps, np.flatnonzero(idx != want)[:8])
    assert np.array_equal(steer_bits, steer_of(want, A).view(np.uint32))


def name_j(u, rnd, greedy_action):
    """A row j (and the row `up` of the next larger draw) whose random action differs from its greedy one, near the median draw."""
    order = np.argsort(u, kind="stable")
    n = len(u)
    for k in list(range(n // 2, n - 1)) + list(range(0, n // 2)):
        j, up = int(order[k]), int(order[k + 1])
        if u[up] > u[j] and rnd[j] != greedy_action[j] and rnd[up] != greedy_action[up]:
            return j, up
    return int(order[n // 2]), None


def seeds(n, k):
    return (0x9E37 * HI) | (17 * n + 1), ((n % 7 + 1) * HI) | (7 * n + 3 + k)


def run_case(rows_kind, mfma, A, dueling, which, sizes):
    f16 = mfma == "f16"
    flat = fresh_flat(A, dueling, 10 * A + dueling) if which == "fresh" else stress_flat(A, dueling)
    net = Net(flat, A, dueling, mfma)
    key = "%s/%s/%s" % (rows_kind, mfma, "4" if A + dueling <= 4 else "NMAX")
    rng = np.random.default_rng([A, int(dueling), len(rows_kind), int(f16), which == "fresh"])
    prow = pool().rows
    for n in sizes:
        obs, code, X = store(prow[rng.integers(0, len(prow), n)], rows_kind)
        r = act_f64(X, flat, n_actions=A, dueling=dueling, eps=0.0, seed=0, counter=0, f16=f16)
        kept = {}
        for k, eps in enumerate((-1.0, 0.0, 0.1, 1.0, "u[j]")):
            seed, counter = seeds(n, k)
            u, rnd = draws(n, seed, counter, A)
            j = up = None
            if eps == "u[j]":
                j, up = name_j(u, rnd, first_argmax(kept["q"]))
                eps = float(u[j])
            idx, st, q = act(net, obs, code, n, eps, seed, counter)
            check_a(key, q, r["Q"], r["q_abs"], say=k == 0)
            check_b(idx, st, q, u, rnd, eps, A)
            assert k == 0 or np.array_equal(q.view(np.uint32), kept["q"].view(np.uint32))      # Q does not depend on the draw
            kept.update(q=q)
            if eps == -1.0:
                assert np.array_equal(idx, first_argmax(q))
            if eps == 1.0:
                assert np.array_equal(idx, rnd)
                kept["one"] = (idx, u, rnd)
            if eps == 0.1:                                  # either output alone, and without q_out: the same results
                i2, _, _ = act(net, obs, code, n, eps, seed, counter, want="i")
                _, s2, _ = act(net, obs, code, n, eps, seed, counter, want="s")
                i3, s3, _ = act(net, obs, code, n, eps, seed, counter, want="is")
                assert np.array_equal(i2, idx) and np.array_equal(s2, st) and np.array_equal(i3, idx) and np.array_equal(s3, st)
            if j is not None:
                assert u[j] == np.float32(eps) and idx[j] == rnd[j]
                if up is not None:
                    assert idx[up] == first_argmax(q)[up] and idx[j] != first_argmax(q)[j]
                    kept["ge"] = (idx, u, rnd, eps)
        if n == 1000:
            mutations(key, rows_kind, mfma, which, X, flat, A, dueling, r, kept)


def mutations(key, rows_kind, mfma, which, X, flat, A, dueling, r, kept):
    """(f): the kernel's outputs against MUTANTS of the f64 side.  Forward mutants must fail (a) at the hard bar alone (flag_f16: at
    an aggregate bar); decision mutants must fail (b).  The ratio recorded per mutant is the smallest, over the cases, of the
    error / bar ratio that rejects it (decision mutants: the share of rows that differ)."""
    f16 = mfma == "f16"
    q = kept["q"]
    W1, b1, W2, b2 = unflatten(flat, 100, 64, A + (1 if dueling else 0))
    col = int(FLAG_COLS[np.argmax(X[:, FLAG_COLS].sum(0))])            # the most often set flag
    live = (forward_f64(X, W1, b1, W2, b2, dueling, A)[0] > 0).mean(0)    # a unit no row activates has no bias to drop
    unit = int(np.argmax(live * np.abs(b1) * np.abs(W2).max(0)))
    out = int(np.argsort(np.abs(b2[:A]), kind="stable")[A // 2])        # the advantage / Q bias of median size
    todo = [("flag_col", col), ("b1", unit), ("b2", out)] + ([("mean_a1", 0)] if dueling else [])
    if not f16:
        todo.append(("flag_f16", 0))
    for mut, arg in todo:
        m = act_f64(X, flat, n_actions=A, dueling=dueling, eps=0.0, seed=0, counter=0, f16=f16, mut=mut, mut_arg=arg)
        hard, rms, mean = ratios(q, m["Q"], r["q_abs"])
        print(key, which, A, dueling, "mutant", mut, "hard %.3f rms %.3f mean %.3f" % (hard, rms, mean))
        if mut != "flag_f16":                               # the hard bar ALONE rejects it
            MUT[mut] = min(MUT.get(mut, np.inf), hard)
            assert hard > 1.0, (key, mut, hard)
            continue
        # flag_f16 (the split layer 1 without its second term) is at most 2^-12 relative per flag weight: far below the hard
        # bar by construction, so the aggregate bars have to see it.  REQUIRED of both packed f32-MFMA forms (k_dqn_act_packed<4>
        # and <NMAX>) on every trained net, at every head; the fresh nets' ratios are recorded (docstring)
        name = "flag_f16 %s %s" % (key, which)
        MUT[name] = min(MUT.get(name, np.inf), max(rms, mean))
        if rows_kind == "packed" and which == "stress":
            assert hard <= 1.0 < max(rms, mean), (key, A, dueling, mut, hard, rms, mean)
    idx, u, rnd = kept["one"]
    seed, counter = seeds(len(u), 3)
    for mut in ("rnd_from_u", "counter_lo", "seed_lo"):
        um, rm = draws(len(u), seed, counter, A, mut=mut)
        bad = float((decide(q, um, rm, 1.0) != idx).mean())
        MUT[mut] = min(MUT.get(mut, np.inf), bad)
        assert bad > 0.25, (mut, bad)
    idx, u, rnd, eps = kept["ge"]
    assert not np.array_equal(decide(q, u, rnd, eps, mut="ge"), idx)


@pytest.mark.parametrize("case", CASES, ids=lambda c: "-".join(str(x) for x in c))
def test_act_against_f64_and_philox(case):
    run_case(*case, sizes=SIZES)


@pytest.mark.parametrize("rows_kind", ["f16", "packed"])
def test_act_h_second_trip_round_its_tile_loop(rows_kind):
    """k_dqn_act_h caps its grid at 512 workgroups: at n = 512 * 64 + 64 + 37 workgroups 0 and 1 take a second tile, the second
    of them ragged."""
    run_case(rows_kind, "f16", 3, False, "stress", sizes=(N_H2,))
    run_case(rows_kind, "f16", 3, True, "fresh", sizes=(N_H2,))


def test_f16_mfma_refuses_what_it_cannot_take():
    L = _lib()
    rows = pool().rows[:64]
    for A, dueling in LARGE:
        net = Net(fresh_flat(A, dueling, 1), A, dueling, "f16")
        for kind in ("f16", "packed"):
            obs, code, _ = store(rows, kind)
            act(net, obs, code, 64, 0.0, 1, 1, expect=L.EINVAL)
    net = Net(fresh_flat(3, False, 1), 3, False, "f16")
    obs, code, _ = store(rows, "f32")
    act(net, obs, code, 64, 0.0, 1, 1, expect=L.EINVAL)
    for A, dueling in ((15, False), (14, True), (1, False)):            # net_ok: 2 <= A, n2 + 2 <= 16
        P = 6464 + (A + dueling) * 65
        net = Net(np.zeros(P, dtype=np.float32), A, dueling, "f32")
        act(net, obs, code, 64, 0.0, 1, 1, expect=L.EINVAL)


TIES = [(3, False, 0, 1), (3, False, 1, 2), (3, True, 0, 2), (9, False, 0, 5), (9, True, 3, 7), (9, True, 0, 8)]


@pytest.mark.parametrize("rows_kind,mfma", FORMS, ids=lambda x: str(x))
def test_exact_ties_take_the_first_maximum(rows_kind, mfma):
    """(c): two identical layer-2 rows and biases, every other action 30 below: the two Q values bit-equal in every row, the lower
    index wins -- and the last-maximum mutant of decide is rejected."""
    rng = np.random.default_rng(8)
    n = 200
    obs, code, X = store(pool().rows[rng.integers(0, len(pool().rows), n)], rows_kind)
    for A, dueling, a, b in TIES:
        if mfma == "f16" and A + dueling > 4:
            continue
        flat = tie_rows(fresh_flat(A, dueling, 3 + A), A, dueling, a, b)
        net = Net(flat, A, dueling, mfma)
        r = act_f64(X, flat, n_actions=A, dueling=dueling, eps=-1.0, seed=0, counter=0, f16=mfma == "f16")
        assert np.allclose(r["Q"][:, a], r["Q"][:, b], rtol=0, atol=1e-12)
        assert np.all(r["Q"][:, a] - np.delete(r["Q"], [a, b], axis=1).max(1) > 20.0)      # the tied pair is the maximum, by far
        seed, counter = seeds(n, A)
        idx, st, q = act(net, obs, code, n, -1.0, seed, counter)
        check_a("%s/%s/ties" % (rows_kind, mfma), q, r["Q"], r["q_abs"])
        assert np.array_equal(q[:, a].view(np.uint32), q[:, b].view(np.uint32))
        assert np.all(q.max(1) == q[:, a])
        assert np.all(idx == a), (A, dueling, a, b, np.unique(idx))
        u, rnd = draws(n, seed, counter, A)
        check_b(idx, st, q, u, rnd, -1.0, A)
        assert np.all(decide(q, u, rnd, -1.0, mut="last_max") == b)


def hand_table(rng, n, A):
    """Q tables with what a scan can get wrong: exact ties (values on a coarse grid), +-inf, all-equal rows."""
    q = rng.normal(0, 3, (n, A)).astype(np.float32)
    kind = rng.integers(0, 6, n)
    q[kind == 1] = np.round(q[kind == 1])                                # many exact ties
    q[kind == 2] = np.float32(rng.normal())                              # all equal
    sel = kind == 3
    q[sel] = np.where(rng.random((sel.sum(), A)) < 0.4, np.float32(np.inf), q[sel])
    sel = kind == 4
    q[sel] = np.where(rng.random((sel.sum(), A)) < 0.6, np.float32(-np.inf), q[sel])
    q[kind == 5, -1] = q[kind == 5].max(1)                              # the last action ties the maximum
    return q


@pytest.mark.parametrize("n", [1, 255, 257, 2048 * 256 + 300])
@pytest.mark.parametrize("A", [2, 3, 9, 14])
def test_select_actions_is_decide(A, n):
    """(d): k_select_actions (what bench.py's torch-learner leg calls) against decide on hand-built tables; its grid is capped at
    2 048 workgroups of 256: n = 2 048 * 256 + 300 takes 300 threads round the loop a second time."""
    lib = _lib().load()
    rng = np.random.default_rng([A, n])
    q = hand_table(rng, n, A)
    qd = torch.tensor(q, device="cuda")
    g = first_argmax(q)
    for k, eps in enumerate((-1.0, 0.0, 0.1, 1.0, "u[j]")):
        seed, counter = seeds(n % 100003, k)
        u, rnd = draws(n, seed, counter, A)
        j = up = None
        if eps == "u[j]":
            j, up = name_j(u, rnd, g)
            eps = float(u[j])
        idx, st, _ = out_bufs(n, A, "is")
        assert lib.uavenv_select_actions(qd.data_ptr(), n, A, eps, seed, counter, idx.data_ptr(), st.data_ptr(), stream()) == 0
        torch.cuda.synchronize()
        idx_h, st_h, _ = read_bufs(n, idx, st, None)
        check_b(idx_h, st_h, q, u, rnd, eps, A)
        if j is not None:
            assert idx_h[j] == rnd[j] and (up is None or idx_h[up] == g[up])
        if k == 2:                                          # either output alone
            i2, s2, _ = out_bufs(n, A, "is")
            assert lib.uavenv_select_actions(qd.data_ptr(), n, A, eps, seed, counter, i2.data_ptr(), None, stream()) == 0
            assert lib.uavenv_select_actions(qd.data_ptr(), n, A, eps, seed, counter, None, s2.data_ptr(), stream()) == 0
            torch.cuda.synchronize()
            i2_h, s2_h, _ = read_bufs(n, i2, s2, None)
            assert np.array_equal(i2_h, idx_h) and np.array_equal(s2_h, st_h)
    assert lib.uavenv_select_actions(qd.data_ptr(), n, A, 0.0, 1, 1, None, None, stream()) == _lib().EINVAL


@pytest.mark.parametrize("rows_kind,A,dueling", [("f32", 3, False), ("packed", 9, True), ("f16", 14, False)])
def test_select_actions_on_the_act_kernels_own_table(rows_kind, A, dueling):
    lib = _lib().load()
    n = 777
    net = Net(stress_flat(A, dueling), A, dueling, "f32")
    obs, code, _ = store(pool().rows[1000:1000 + n], rows_kind)
    seed, counter = seeds(n, 0)
    idx, st, q = act(net, obs, code, n, 0.3, seed, counter)
    qd = torch.tensor(q, device="cuda")
    i2 = torch.full((n,), -7, dtype=torch.int32, device="cuda")
    s2 = torch.full((n,), float("nan"), device="cuda")
    assert lib.uavenv_select_actions(qd.data_ptr(), n, A, 0.3, seed, counter, i2.data_ptr(), s2.data_ptr(), stream()) == 0
    torch.cuda.synchronize()
    assert np.array_equal(i2.cpu().numpy(), idx) and np.array_equal(s2.cpu().numpy().view(np.uint32), st)
    assert 0 < (idx != first_argmax(q)).sum() < n


class _Shim:
    def __init__(self, net):
        self.net = net.net


@pytest.mark.parametrize("launch,N", [("coop", 64), ("coop", 1000), ("polh", 962)])
def test_in_step_policy_takes_the_act_kernels_actions(launch, N):
    """(e): uavenv_step_policy / uavenv_step_policy_img on freshly reset agents: packed envs through k_step_coop<.., POLICY> (f32
    MFMA, with and without the layer-1 image), an f16 env through the one-wave k_step_polh (f16 MFMA).  The call must be TAKEN
    (True: no fall-back to act + step); the action plane it writes equals uavenv_dqn_act's index_out on the same current rows
    for every agent the step reports valid; and that index_out is held to f64 and the oracle's stream right here."""
    from dqn_based_uav_3d_path_planer_amd import _lib as L
    from dqn_based_uav_3d_path_planer_amd.data import make_city26_env
    from dqn_based_uav_3d_path_planer_amd.replay import DeviceReplayRing
    polh = launch == "polh"
    env = make_city26_env(N, obs_dtype=torch.float16 if polh else "packed")
    ring = DeviceReplayRing(env, 2 * N, discrete=True)
    if polh:
        ring.extra_flags = L.STEP_ONE_WAVE
    code = L.OBS_F16 if polh else L.OBS_PACKED
    key = "step %s" % launch
    for dueling in (False, True):
        for which in ("fresh", "stress"):
            flat = fresh_flat(3, dueling, 21) if which == "fresh" else stress_flat(3, dueling)
            net = Net(flat, 3, dueling, "f16" if polh else "f32")
            for use_img in ((False,) if polh else (False, True)):
                img = net.image() if use_img else None
                assert img is None or img.data_ptr() % 16 == 0          # (a misaligned image is dropped by the launch)
                for k, eps in enumerate((-1.0, 0.0, 0.1, 1.0, "u[j]")):
                    ring.reset(seed=3 + k)
                    cur = ring.current_obs()
                    X = (cur.float().cpu().numpy() if polh else unpack(cur[None])[0]).astype(np.float64)
                    seed, counter = seeds(N, k)
                    u, rnd = draws(N, seed, counter, 3)
                    r = act_f64(X, flat, n_actions=3, dueling=dueling, eps=0.0, seed=0, counter=0, f16=polh)
                    if eps == "u[j]":
                        eps = float(u[name_j(u, rnd, r["index"])[0]])
                    idx, st, q = act(net, cur, code, N, eps, seed, counter)
                    check_a(key, q, r["Q"], r["q_abs"], say=k == 0)
                    check_b(idx, st, q, u, rnd, eps, 3)
                    ring.action[0].fill_(-7)                          # the plane holds nothing the launch did not write
                    assert ring.step_policy(_Shim(net), eps, seed, counter, auto_reset=False, image=img) is True
                    torch.cuda.synchronize()
                    valid = ring.valid[0].cpu().numpy() != 0
                    assert valid.sum() > N // 2
                    plane = ring.action[0].cpu().numpy()
                    assert np.all((plane >= 0) & (plane < 3))
                    assert np.array_equal(plane[valid], idx[valid]), (launch, N, dueling, which, use_img, eps)
                    if eps == 0.1:
                        assert len(np.unique(plane)) == 3
    env.close()
