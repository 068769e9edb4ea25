"""Directed worlds and positions for the 80 occupancy flags of state_PathPlan (Agents/UAV.py:533-566).

Shared by tests/test_stencil_edges.py (host) and tests/test_stencil_edges_gpu.py (device).  No GPU here.

The device reaches the flags through conservative shortcuts (csrc/uavenv_device.hpp): per-cell candidate masks with
halos, a quick reject / quick accept per (cylinder, stencil), and a threshold that replaces the square root.  Those
decide something only when a stencil point lies within rounding of a rim, a stencil corner within rounding of the
reject / accept radius, a coordinate on a box face or a cell edge, or the height on a roof.  A uniform draw never gets
there; the catalogue built here is made of nothing else:

  edge_world(cell, wide)      <= 64 cylinders: radii on both sides of 2*sqrt(2)*spacing, roofs at 0 / mid / box height
                              / above, cylinders across every map edge, cylinders tangent to the reach of a stencil that
                              is anchored on a cell edge; wide = more than 32 of them (64-bit masks)
  edge_positions(b, cell)     flip pairs (adjacent doubles across a rim, by bisection with the reference's own test), the
                              same at roof heights, box faces, cell edges
  oracle_flags(world, pos)    the 80 expected flags: 80 calls of Threaten_rate on the probe points of
                              oracle/uav_oracle.c:273-287
  queue_world / queue_positions / full_triples      a crowd that fills the per-wavefront stencil queue several times
  lattice_world / lattice_positions                 the same load with one disc per stencil point: every queue item owns a flag
"""
import numpy as np

W = 500.0          # Envs/PathPlan_City.py: x and y are both bounded by `width`
HBOX = 100.0
SPACINGS = (1.0, 5.0, 10.0)
FLAG_COLS = np.r_[11:86, 90:95]          # the 75 stencil flags and the 5 below-probes in a 100-column observation
TANGENT_D = (0.0, 1e-9, -1e-9, 1e-7, -1e-7)
TANGENT_R, TANGENT_H = 3.0, 50.0

_INF = np.inf


def _tangent_setups(cell):
    """[(cylinder row, agent x on the cell edge, agent y, spacing)]: the rim of each cylinder is tangent (to d) to the
    left-most column of a stencil whose centre sits on the cell edge X = ix * cell:  cx = X - 2 sp - R + d."""
    out = []
    lanes = {1.0: (170.0, 30.0, 48.0, 0), 5.0: (170.0, 30.0, 48.0, 5), 10.0: (330.0, 60.0, 80.0, 0)}
    for sp in SPACINGS:
        y, x_first, pitch, slot0 = lanes[sp]
        for q, d in enumerate(TANGENT_D):
            ix = int(np.ceil((x_first + pitch * (slot0 + q)) / cell))
            X = ix * cell
            cy = y + 0.37 * q
            out.append(([X - 2.0 * sp - TANGENT_R + d, cy, 0.0, TANGENT_R, TANGENT_H], X, cy, sp))
    return out


def edge_world(cell, wide=False):
    """-> [nb, 5] rows [cx, cy, 0, R, H]; nb = 29 (u32 masks), or 40 with wide=True (u64 masks).  In either the cylinders
    tangent to the widest stencil's reach (the ones only the 20 m halo lists) hold the first and the last index; in the
    wide world also 31 and 32, the two sides of the mask's word boundary."""
    return _edge_world(cell, wide)[0]


def _edge_world(cell, wide):
    """-> (rows, is_filler [nb] bool)."""
    mid = 37.5
    radii = [(90.37, 90.21, 2.82), (250.12, 90.4, 2.83), (410.3, 90.7, 0.5),
             (90.2, 250.6, 28.28), (250.0, 250.9, 14.15), (410.8, 250.1, 14.14),
             (90.9, 410.3, 28.29), (250.4, 410.2, 40.0), (410.6, 410.0, 55.0)]
    heights = [0.0, mid, HBOX, 120.0]
    rows = [[cx, cy, 0.0, R, heights[k % 4]] for k, (cx, cy, R) in enumerate(radii)]
    rows[7][4], rows[8][4] = mid, HBOX                               # the two large discs: under and at the box height
    rows += [[-3.0, 250.3, 0.0, 10.0, 120.0],                         # centre outside the box, across x = 0
             [498.5, 60.2, 0.0, 8.0, HBOX],                           # across x = W
             [333.1, 1.2, 0.0, 9.0, mid],                             # across y = 0
             [120.9, 499.5, 0.0, 7.0, 0.0],                           # across y = W
             [0.7, 0.4, 0.0, 12.0, 60.0]]                             # over the corner (0, 0)
    tang = _tangent_setups(cell)
    t10 = [t[0] for t in tang if t[3] == 10.0]
    rows += [t[0] for t in tang if t[3] != 10.0]
    n_plain = len(rows)
    if wide:                                                          # eleven small fillers in a free row
        rows += [[30.0 + 40.0 * k, 30.0 + 0.1 * k, 0.0, 1.5 + 0.2 * k, heights[k % 4]] for k in range(11)]
    nb = len(rows) + len(t10)
    at = [0, 31, 32, nb - 1, 16] if wide else [0, nb - 1, 9, 16, 23]
    out, filler = [None] * nb, np.zeros(nb, dtype=bool)
    for k, p in enumerate(at):
        out[p] = t10[k]
    rest = iter(enumerate(rows))
    for p in range(nb):
        if out[p] is None:
            k, out[p] = next(rest)
            filler[p] = k >= n_plain
    b = np.asarray(out, dtype=np.float64)
    assert len(b) <= 64 and (len(b) > 32) == bool(wide)
    return b, filler


def tangent_agents(buildings, cell):
    """[(x on the cell edge, y, index of the tangent cylinder, spacing)] of edge_world(cell, ...) == buildings."""
    out = []
    for row, X, cy, sp in _tangent_setups(cell):
        hit = np.nonzero((buildings[:, 0] == row[0]) & (buildings[:, 1] == row[1]))[0]
        assert len(hit) == 1
        out.append((X, cy, int(hit[0]), sp))
    return out


def _inside(x, y, cx, cy, R):
    """The reference's own test (Obstacles/building.py:20-26, below the roof): sqrt(dx^2 + dy^2 + 0) < R."""
    return np.sqrt((x - cx) ** 2 + (y - cy) ** 2) < R


# the stencil points a flip is aimed through: corners, centre, edge midpoints, one asymmetric point
FLIP_POINTS = ((0, 0), (0, 4), (4, 0), (4, 4), (2, 2), (0, 2), (2, 0), (4, 2), (2, 4), (1, 3))
# the eight multiples of pi/4 and two oblique directions
FLIP_DIRS = tuple(k * np.pi / 4 for k in range(8)) + (0.3, 2.0)


def flip_pairs(buildings, cyl=None, dirs=FLIP_DIRS):
    """Per (cylinder, spacing, stencil point (i, j), direction): the agent starts where probe (i, j) sits on the cylinder's
    centre and moves along the ray; bisection on the ray parameter, in float64 and with the probe point formed as the
    observation forms it (p + sp * (i - 2)), until two adjacent parameters give different results of `_inside`.
    -> (inner [m, 2], outer [m, 2], inner_nb [m, 2], outer_nb [m, 2], H [m]): the two agent positions of the flip, and
    the neighbouring doubles one step further in and out along the ray.  A corner point on its own diagonal flips at
    exactly the reject radius R + 2 sqrt(2) sp (outward corner) or the accept radius R - 2 sqrt(2) sp (trailing corner)."""
    cyl = range(len(buildings)) if cyl is None else cyl
    rec = [(b, sp, i, j, th) for b in cyl for sp in SPACINGS for (i, j) in FLIP_POINTS for th in dirs]
    bi = np.array([r[0] for r in rec])
    sp = np.array([r[1] for r in rec])
    ox, oy = sp * (np.array([r[2] for r in rec]) - 2.0), sp * (np.array([r[3] for r in rec]) - 2.0)
    th = np.array([r[4] for r in rec])
    ux, uy = np.cos(th), np.sin(th)
    ux[np.abs(ux) < 1e-15] = 0.0
    uy[np.abs(uy) < 1e-15] = 0.0
    cx, cy, R, H = buildings[bi, 0], buildings[bi, 1], buildings[bi, 3], buildings[bi, 4]
    x0, y0 = cx - ox, cy - oy

    def pos(t):
        return x0 + t * ux, y0 + t * uy

    def inside(t):
        px, py = pos(t)
        return _inside(px + ox, py + oy, cx, cy, R)

    lo, hi = np.zeros(len(rec)), 2.0 * R + 1.0
    assert inside(lo).all() and not inside(hi).any()
    while True:
        mid = lo + (hi - lo) / 2
        open_ = (mid > lo) & (mid < hi)
        if not open_.any():
            break
        m_in = inside(mid)
        lo = np.where(open_ & m_in, mid, lo)
        hi = np.where(open_ & ~m_in, mid, hi)
    assert np.array_equal(np.nextafter(lo, _INF), hi)
    pin, pout = np.stack(pos(lo), 1), np.stack(pos(hi), 1)
    u = np.stack([ux, uy], 1)
    step = np.where(u > 0, _INF, np.where(u < 0, -_INF, 0.0))
    far = lambda p, s: np.where(s == 0.0, p, np.nextafter(p, s))    # noqa: E731
    return pin, pout, far(pin, -step), far(pout, step), H


def _with_z(xy, z):
    xy = np.asarray(xy, dtype=np.float64).reshape(-1, 2)
    return np.c_[xy, np.broadcast_to(np.asarray(z, dtype=np.float64), (len(xy),))]


def edge_positions(buildings, cell, seed=5):
    """-> ([n, 3] float64 positions, {kind: slice}) for edge_world(cell, ...) == buildings.  No x or y is -0.0 (a move by
    +0.0 would turn it into +0.0, and the device tests assert positions bit for bit)."""
    rng = np.random.default_rng(seed)
    parts, kinds = [], {}

    def add(kind, p):
        p = np.asarray(p, dtype=np.float64).reshape(-1, 3)
        at = sum(len(q) for q in parts)
        parts.append(p)
        lo = kinds[kind].start if kind in kinds else at
        kinds[kind] = slice(lo, at + len(p))

    # ---- flip pairs on the ground, and the two doubles of each flip at the roof's heights.  The eleven small fillers of
    # the wide world get four of the ten directions.
    again, is_filler = _edge_world(cell, len(buildings) > 32)
    assert np.array_equal(again, buildings), "edge_positions wants edge_world(cell, ...) of the same cell"
    sets = [flip_pairs(buildings, np.nonzero(~is_filler)[0])]
    if is_filler.any():
        sets.append(flip_pairs(buildings, np.nonzero(is_filler)[0], dirs=FLIP_DIRS[1:8:2]))
    pin, pout, pin2, pout2, H = (np.concatenate(c) for c in zip(*sets))
    add("flip", np.r_[_with_z(pin, 0.0), _with_z(pout, 0.0), _with_z(pin2, 0.0), _with_z(pout2, 0.0)])
    for z in (H, np.nextafter(H, _INF), H + 1.0, H + 3.0):          # (pz = 0 is the ground pass above)
        add("flip_at_height", np.r_[np.c_[pin, z], np.c_[pout, z]])

    # ---- box faces: a stencil row / column exactly on x = 0 or x = W (and y), with both neighbours; then both together
    zs = [-5e-324, -0.0, 0.0, 1.0, 5.0, np.nextafter(5.0, 0.0), 100.0, np.nextafter(100.0, _INF), 101.0, 104.0, 105.0,
          np.nextafter(105.0, _INF)]
    face = []
    for sp in SPACINGS:
        for i in range(5):
            for e in (0.0, W):
                v = e - sp * (i - 2)
                face += [np.nextafter(v, -_INF), v, np.nextafter(v, _INF)]
    face = np.asarray(face)
    assert not np.signbit(face[face == 0.0]).any()
    for z in zs:
        other = rng.uniform(-25.0, 525.0, len(face))
        add("box_face", np.c_[face, other, np.full(len(face), z)])
        other = rng.uniform(-25.0, 525.0, len(face))
        add("box_face", np.c_[other, face, np.full(len(face), z)])
        add("box_face", np.c_[face, face, np.full(len(face), z)])
        add("box_face", np.c_[face, face[::-1], np.full(len(face), z)])

    # ---- cell edges: where the truncation and the clamp of cell_of decide the mask that is read
    gn = max(1, int(np.ceil(W / cell)))
    edges = np.arange(gn + 1) * cell
    edges = np.r_[np.nextafter(edges, -_INF), edges, np.nextafter(edges, _INF)]
    for rep in range(3):
        add("cell_edge", np.c_[edges, rng.uniform(-5.0, 505.0, len(edges)), np.zeros(len(edges))])
        add("cell_edge", np.c_[rng.uniform(-5.0, 505.0, len(edges)), edges, np.full(len(edges), 10.0 * rep)])
    add("cell_edge", np.c_[edges, edges, np.zeros(len(edges))])
    for X, cy, b, sp in tangent_agents(buildings, cell):
        for x in (np.nextafter(X, -_INF), X, np.nextafter(X, _INF)):
            for z in (0.0, TANGENT_H, np.nextafter(TANGENT_H, _INF)):
                add("tangent", [x, cy, z])
                add("tangent", [x, np.nextafter(cy, _INF), z])
    pos = np.concatenate(parts)
    assert not (np.signbit(pos[:, :2]) & (pos[:, :2] == 0.0)).any()
    return pos, kinds


def probe_points(positions):
    """[n, 80, 3]: the probe points as oracle/uav_oracle.c:273-287 forms them (p + d for spacing 1, p + scale * d otherwise,
    i over x and j over y; then (px, py, pz - k), k = 1..5)."""
    p = np.asarray(positions, dtype=np.float64).reshape(-1, 3)
    n = len(p)
    out = np.empty((n, 80, 3))
    d = np.arange(5.0) - 2.0
    for s, scale in enumerate(SPACINGS):
        off = d if s == 0 else scale * d
        for i in range(5):
            for j in range(5):
                c = 25 * s + 5 * i + j
                out[:, c, 0] = p[:, 0] + off[i]
                out[:, c, 1] = p[:, 1] + off[j]
                out[:, c, 2] = p[:, 2]
    for k in range(1, 6):
        out[:, 74 + k, 0] = p[:, 0]
        out[:, 74 + k, 1] = p[:, 1]
        out[:, 74 + k, 2] = p[:, 2] - float(k)
    return out


def oracle_flags(world, positions, chunk=16384):
    """-> [n, 80] uint8: the 75 stencil flags then the 5 below-probes, by OracleWorld.threaten_rate_many on the 80 probe
    points of every position."""
    p = np.asarray(positions, dtype=np.float64).reshape(-1, 3)
    out = np.empty((len(p), 80), dtype=np.uint8)
    for lo in range(0, len(p), chunk):
        pts = probe_points(p[lo:lo + chunk])
        out[lo:lo + chunk] = world.threaten_rate_many(pts.reshape(-1, 3)).reshape(-1, 80).astype(np.uint8)
    return out


# ---------------------------------------------------------------------------------------------- the queue's crowd
QUEUE_PATCH = (247.0, 247.0, 6.0)           # x0, y0, side
QUEUE_FAR = (403.0, 77.0, 10.0)             # an agent here reads an empty mask and flies over nothing


def queue_world():
    """64 cylinders of R in [1, 2] with their centres in the 6 m patch, roofs at 30: every mask bit, the six-bit cylinder
    field of a queue item up to 63."""
    rng = np.random.default_rng(12)
    x0, y0, side = QUEUE_PATCH
    nb = 64
    b = np.c_[x0 + rng.uniform(0.0, side, nb), y0 + rng.uniform(0.0, side, nb), np.zeros(nb), rng.uniform(1.0, 2.0, nb),
              np.full(nb, 30.0)]
    dist = np.hypot(b[:, 0] - QUEUE_FAR[0], b[:, 1] - QUEUE_FAR[1])
    assert (dist > 100.0).all()
    return b


def queue_positions():
    """[64, 3]: an 8 x 8 lattice inside the patch, on the ground (below every roof)."""
    x0, y0, side = QUEUE_PATCH
    t = (np.arange(8.0) + 0.5) * (side / 8.0)
    gx, gy = np.meshgrid(x0 + t, y0 + t * 0.97, indexing="ij")
    return np.c_[gx.ravel(), gy.ravel(), np.zeros(64)]


# In the crowd every stencil point lies under several discs at once, so a queue item that went missing would usually
# be covered by another item's bits.  The lattice is the opposite: 41 discs that sit ON the stencil points of an agent
# near the centre -- one disc per point of the 5 m stencil, one per point of the 10 m stencil -- so that every item owns
# a flag no other item sets.  The queues fill as well (51 triples per agent), and one lost item is one wrong flag.
LATTICE_CENTRE = (251.0, 249.0)


def lattice_world():
    cx0, cy0 = LATTICE_CENTRE
    at = [(5.0 * i, 5.0 * j) for i in range(-2, 3) for j in range(-2, 3)]
    at += [(10.0 * i, 10.0 * j) for i in range(-2, 3) for j in range(-2, 3) if max(abs(i), abs(j)) == 2]
    b = np.array([[cx0 + dx, cy0 + dy, 0.0, 1.5 + 0.01 * (k % 40), 30.0] for k, (dx, dy) in enumerate(at)])
    assert len(b) == 41 and len({(r[0], r[1]) for r in b.tolist()}) == 41
    return b


def lattice_positions():
    """[64, 3]: an 8 x 8 lattice within 0.6 m of the centre, on the ground: every stencil point of the 5 m and 10 m
    stencils is inside its own disc (R >= 1.5), and inside no other."""
    cx0, cy0 = LATTICE_CENTRE
    t = (np.arange(8.0) - 3.5) * (1.2 / 8.0)
    gx, gy = np.meshgrid(cx0 + t, cy0 + t * 0.93, indexing="ij")
    return np.c_[gx.ravel(), gy.ravel(), np.zeros(64)]


def full_triples(buildings, positions, cylinders=None):
    """Per agent: the number of (cylinder, spacing) pairs whose 25 stencil points are neither all inside nor all outside
    the disc, with the agent not above the roof.  A geometric statement (the reference's own point test on the 25 points),
    made without the device's guards: such a pair can be neither quickly accepted nor quickly rejected, so it is a lower
    bound on what any correct classifier must hand to the exact 25-point test."""
    p = np.asarray(positions, dtype=np.float64).reshape(-1, 3)
    b = np.asarray(buildings, dtype=np.float64)
    b = b if cylinders is None else b[np.asarray(cylinders)]
    d = np.arange(5.0) - 2.0
    count = np.zeros(len(p), dtype=np.int64)
    for sp in SPACINGS:
        x = p[:, None, None, 0] + sp * d[None, None, :]                      # [n, 1, 5]
        y = p[:, None, None, 1] + sp * d[None, None, :]
        dx2 = (x - b[None, :, None, 0]) ** 2                                # [n, nb, 5]
        dy2 = (y - b[None, :, None, 1]) ** 2
        ins = np.sqrt(dx2[:, :, :, None] + dy2[:, :, None, :]) < b[None, :, None, None, 3]
        k = ins.reshape(len(p), len(b), 25).sum(axis=2)
        low = ~(p[:, None, 2] > b[None, :, 4])
        count += ((k > 0) & (k < 25) & low).sum(axis=1)
    return count
