"""The observation stencils' design against the oracle at every geometric edge -- host only.

A numpy restatement of the tables of uavenv_set_buildings (csrc/uavenv.hip) and of obs_bits (csrc/uavenv_device.hpp):

  thr    the smallest double whose rounded square root reaches R, by the nextafter loop;
  rej2   (R + 2 sqrt(2) sp + 1e-6)^2, acc2 (R - 2 sqrt(2) sp - 1e-6)^2 or -1;
  grids  three candidate masks per cell, halo 2 / 10 / 20 m plus the 1e-6-scale margins;
  cell   truncation of x * (1 / cell), clamped into the grid;

is held to tests/stencil_edges.oracle_flags (80 calls of the oracle's Threaten_rate per position) on the catalogue of
tests/stencil_edges.py: every flag equal, for the 29-cylinder world (32-bit masks) at cell 20 and the 40-cylinder world
(64-bit masks) at cell 13, whose reciprocal is inexact.  tests/test_stencil_edges_gpu.py then holds the four device
texts to the same expected flags.

Then each of seven small mutations of the restatement must change at least one flag, which shows that the catalogue can
see an error of that size.  The two guard mutations are stated against the GEOMETRIC radius: the reject radius as
R + 2 sqrt(2) sp - 1e-9 and the accept radius as R - 2 sqrt(2) sp + 1e-9.  (Taking 1e-9 off the guarded radius
R + 2 sqrt(2) sp + 1e-6 changes no flag anywhere, by design: that is what the guard is for.  Likewise a halo short by less
than the masks' two margins is not detectable and not asked for.)

Positions of the catalogue that each mutation changes (40-cylinder world, cell 13, 125 670 positions), as printed by
test_catalogue_rejects_the_mutation:

  thr = R * R                      250
  thr one ulp up                 7 587
  reject radius 1e-9 short       1 406
  accept radius 1e-9 long          435
  20 m halo as 19.99 m              34
  pz >= H for pz > H            26 132
  x >= W for x > W in the box      476

Catalogue sizes: 109 536 positions (29 cylinders, cell 20), 125 670 (40 cylinders, cell 13).  The module takes about
15 s, most of it the oracle's 80 probes per position.
"""
import functools

import numpy as np
import pytest

import stencil_edges as se

HALOS = (2.0, 10.0, 20.0)


def build_tables(buildings, cell, *, thr_mode="exact", rej_radius=None, acc_radius=None, halo20=20.0):
    """uavenv_set_buildings, restated.  The keyword arguments are the mutations."""
    b = np.asarray(buildings, dtype=np.float64)
    nb = len(b)
    R = b[:, 3]
    thr = np.zeros(nb)
    for i in range(nb):
        t = R[i] * R[i]
        if R[i] > 0:
            while np.sqrt(t) >= R[i]:
                t = np.nextafter(t, -np.inf)
            while np.sqrt(t) < R[i]:
                t = np.nextafter(t, np.inf)
        else:
            t = 0.0
        thr[i] = t
    if thr_mode == "square":
        thr = R * R
    elif thr_mode == "ulp_up":
        thr = np.nextafter(thr, np.inf)
    rej2, acc2 = np.zeros((nb, 3)), np.zeros((nb, 3))
    for k, sp in enumerate(se.SPACINGS):
        diag, guard = 2.0 * np.sqrt(2.0) * sp, 1e-6
        ro = R + diag + guard if rej_radius is None else rej_radius(R, diag)
        ri = R - diag - guard if acc_radius is None else acc_radius(R, diag)
        rej2[:, k] = np.where(ro > 0, ro * ro, 0.0)
        acc2[:, k] = np.where(ri > 0, ri * ri, -1.0)
    gn = max(1, int(np.ceil(se.W / cell)))
    margin = 1e-6 * (cell if cell > 1.0 else 1.0)
    ix = np.arange(gn, dtype=np.float64)
    grids = []
    for halo in (HALOS[0], HALOS[1], halo20):
        lo, hi = ix * cell - halo - margin, (ix + 1.0) * cell + halo + margin
        m = np.zeros((gn, gn), dtype=np.uint64)                              # [iy, ix]
        for i in range(nb):
            qx = np.clip(b[i, 0], lo, hi)
            qy = np.clip(b[i, 1], lo, hi)
            d = np.hypot(qx[None, :] - b[i, 0], qy[:, None] - b[i, 1])
            m |= np.where(d < R[i] + margin, np.uint64(1) << np.uint64(i), np.uint64(0))
        grids.append(m.ravel())
    return dict(cx=b[:, 0], cy=b[:, 1], thr=thr, H=b[:, 4], rej2=rej2, acc2=acc2, g=grids, gn=gn, inv_cell=1.0 / cell, nb=nb)


def cell_of(t, x, y):
    gn = t["gn"]
    ix = np.clip(np.trunc(x * t["inv_cell"]), 0, gn - 1).astype(np.int64)
    iy = np.clip(np.trunc(y * t["inv_cell"]), 0, gn - 1).astype(np.int64)
    return iy * gn + ix


def obs_bits(t, pos, *, roof_ge=False, box_ge=False):
    """obs_bits of csrc/uavenv_device.hpp, restated -> [n, 80] uint8.  roof_ge / box_ge are mutations."""
    px, py, pz = pos[:, 0], pos[:, 1], pos[:, 2]
    n = len(pos)
    d = np.arange(5.0) - 2.0
    over = (lambda v: v >= se.W) if box_ge else (lambda v: v > se.W)
    above = (lambda z, H: z >= H) if roof_ge else (lambda z, H: z > H)
    z_out = (pz < 0.0) | (pz > se.HBOX)
    bits = np.zeros((3, n, 5, 5), dtype=bool)
    for k, sp in enumerate(se.SPACINGS):
        xi, yi = px[:, None] + sp * d[None, :], py[:, None] + sp * d[None, :]
        bits[k] |= ((xi < 0.0) | over(xi))[:, :, None]
        bits[k] |= ((yi < 0.0) | over(yi))[:, None, :]
        bits[k] |= z_out[:, None, None]
    xy_out = (px < 0.0) | over(px) | (py < 0.0) | over(py)
    zk = pz[:, None] - np.arange(1.0, 6.0)[None, :]
    bl = xy_out[:, None] | (zk < 0.0) | (zk > se.HBOX)
    need_below = ~bl.all(axis=1)
    m = t["g"][2][cell_of(t, px, py)]
    for b in range(t["nb"]):
        sel = np.nonzero((m >> np.uint64(b)) & np.uint64(1))[0]
        if not len(sel):
            continue
        x, y, z = px[sel], py[sel], pz[sel]
        dcx, dcy = x - t["cx"][b], y - t["cy"][b]
        dc2 = dcx * dcx + dcy * dcy
        under = need_below[sel] & (dc2 < t["thr"][b])
        bl[sel] |= under[:, None] & ~above(zk[sel], t["H"][b])
        low = ~above(z, t["H"][b])
        for k, sp in enumerate(se.SPACINGS):
            touch = low & ~(dc2 >= t["rej2"][b, k])
            acc = touch & (dc2 < t["acc2"][b, k])
            bits[k][sel[acc]] = True
            full = np.nonzero(touch & ~acc)[0]
            if len(full):
                dx = (x[full, None] + sp * d[None, :]) - t["cx"][b]
                dy = (y[full, None] + sp * d[None, :]) - t["cy"][b]
                bits[k][sel[full]] |= (dx * dx)[:, :, None] + (dy * dy)[:, None, :] < t["thr"][b]
    return np.concatenate([bits[0].reshape(n, 25), bits[1].reshape(n, 25), bits[2].reshape(n, 25), bl], axis=1).astype(np.uint8)


@functools.lru_cache(maxsize=None)
def _catalogue(wide, cell):
    from oracle import pyoracle as po
    b = se.edge_world(cell, wide)
    pos, kinds = se.edge_positions(b, cell)
    want = se.oracle_flags(po.OracleWorld(b), pos)
    return dict(b=b, cell=cell, pos=pos, kinds=kinds, want=want, wide=wide)


@pytest.fixture(scope="module", params=[(False, 20.0), (True, 13.0)], ids=["u32-cell20", "u64-cell13"])
def catalogue(request):
    return _catalogue(*request.param)


def test_edge_world_is_what_the_catalogue_needs():
    for wide, cell in ((False, 20.0), (True, 13.0), (True, 7.3), (False, 12.5)):
        b = se.edge_world(cell, wide)
        assert (len(b) > 32) == wide and len(b) <= 64
        for R in (2.82, 2.83, 14.14, 14.15, 28.28, 28.29, 0.5, 40.0, 55.0):
            assert (b[:, 3] == R).any()
        assert {0.0, se.HBOX, 120.0} <= set(b[:, 4]) and ((b[:, 4] > 0) & (b[:, 4] < se.HBOX)).any()
        assert (b[:, 0] < 0).any()
        for lo, hi in ((b[:, 0] - b[:, 3], b[:, 0] + b[:, 3]), (b[:, 1] - b[:, 3], b[:, 1] + b[:, 3])):
            assert ((lo < 0) & (hi > 0)).any() and ((lo < se.W) & (hi > se.W)).any()
        t10 = sorted(i for _, _, i, sp in se.tangent_agents(b, cell) if sp == 10.0)
        assert t10[0] == 0 and t10[-1] == len(b) - 1 and (not wide or {31, 32} <= set(t10))
        for X, cy, i, sp in se.tangent_agents(b, cell):
            assert X == round(X / cell) * cell and b[i, 1] == cy
            assert abs((X - 2 * sp) - (b[i, 0] + b[i, 3])) <= 1.001e-7


def test_catalogue_holds_every_kind(catalogue):
    pos, kinds, want = catalogue["pos"], catalogue["kinds"], catalogue["want"]
    assert set(kinds) == {"flip", "flip_at_height", "box_face", "cell_edge", "tangent"}
    assert sum(s.stop - s.start for s in kinds.values()) == len(pos)
    print(f"catalogue {'u64' if catalogue['wide'] else 'u32'} cell {catalogue['cell']}: {len(pos)} positions",
          {k: s.stop - s.start for k, s in kinds.items()})
    f = kinds["flip"]
    m = (f.stop - f.start) // 4
    flip_in, flip_out = want[f.start:f.start + m], want[f.start + m:f.start + 2 * m]
    assert (flip_in != flip_out).any(axis=1).mean() > 0.5            # most flips are visible (the rest: another disc covers them)
    assert 0 < want[:, 75:].mean() < 1 and 0 < want[:, :75].mean() < 1


def test_restatement_equals_the_oracle_on_the_catalogue(catalogue):
    t = build_tables(catalogue["b"], catalogue["cell"])
    got = obs_bits(t, catalogue["pos"])
    bad = np.nonzero((got != catalogue["want"]).any(axis=1))[0]
    assert len(bad) == 0, (len(bad), catalogue["pos"][bad[:5]].tolist())


MUTATIONS = {
    "thr = R * R": (dict(thr_mode="square"), {}),
    "thr one ulp up": (dict(thr_mode="ulp_up"), {}),
    "reject radius 1e-9 short": (dict(rej_radius=lambda R, diag: R + diag - 1e-9), {}),
    "accept radius 1e-9 long": (dict(acc_radius=lambda R, diag: R - diag + 1e-9), {}),
    "20 m halo as 19.99 m": (dict(halo20=19.99), {}),
    "pz >= H for pz > H": ({}, dict(roof_ge=True)),
    "x >= W for x > W in the box": ({}, dict(box_ge=True)),
}


@pytest.mark.parametrize("name", list(MUTATIONS))
def test_catalogue_rejects_the_mutation(name):
    catalogue = _catalogue(True, 13.0)
    tab_kw, obs_kw = MUTATIONS[name]
    got = obs_bits(build_tables(catalogue["b"], catalogue["cell"], **tab_kw), catalogue["pos"], **obs_kw)
    changed = int((got != catalogue["want"]).any(axis=1).sum())
    print(f"mutation {name!r}: {changed} positions rejected")
    assert changed > 0


def test_queue_crowd_precondition_holds_on_the_host():
    b, p = se.queue_world(), se.queue_positions()
    assert len(b) >= 40 and ((b[:, 3] >= 1) & (b[:, 3] <= 2)).all() and (p[:, 2] < b[:, 4].min()).all()
    x0, y0, side = se.QUEUE_PATCH
    for a in (b, p):
        assert ((a[:, 0] >= x0) & (a[:, 0] <= x0 + side) & (a[:, 1] >= y0) & (a[:, 1] <= y0 + side)).all()
    total = int(se.full_triples(b, p).sum())
    per_phase = [int(se.full_triples(b, p, np.arange(ph, len(b), 3)).sum()) for ph in range(3)]
    print("queue crowd: triples per 64 agents", total, "per candidate phase", per_phase)
    assert total >= 4 * 512 and min(per_phase) >= 4 * 512 / 3


def test_queue_lattice_gives_every_triple_a_flag_of_its_own():
    """The second queue world: 51 triples per agent, and the 50 of the two wide stencils set 50 different flags."""
    from oracle import pyoracle as po
    b, p = se.lattice_world(), se.lattice_positions()
    assert ((b[:, 3] >= 1) & (b[:, 3] <= 2)).all() and (p[:, 2] < b[:, 4].min()).all()
    tri = se.full_triples(b, p)
    per_phase = [int(se.full_triples(b, p, np.arange(ph, len(b), 3)).sum()) for ph in range(3)]
    assert (tri == 51).all() and tri.sum() >= 4 * 512 and min(per_phase) >= 4 * 512 / 3
    want = se.oracle_flags(po.OracleWorld(b), p)
    assert want[:, 25:75].all() and not want[:, :25].all(axis=1).any()     # (the 1 m stencil is partly free)
