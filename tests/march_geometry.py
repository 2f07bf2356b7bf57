"""The launch geometry of the x-step's z-marching kernels, restated (pure Python, no GPU), and what the seam tests share.

`geometry` follows march_geom (csrc/kernels_cds.hip: k_cds_march, 512 threads, chunks of SIPX_CDS_MARCH_ZCHUNK planes) and the
tile part of try_rhs_march (csrc/kernels_sets.hip: k_rhs_march, 256 threads, SIPX_RHS_MARCH_ZCHUNK) line by line, both forced
(SIPX_CDS_MARCH=2 / SIPX_RHS_MARCH=2).  TABLE lists the small grids the seam tests run on with the properties each is there
for, per kernel and precision; tests/test_gpu_march_seams.py proves every listed property on the CPU, so a change of a tile
constant fails there instead of silently moving a seam off the grid.

Also here: the route counters of kernel_stats_all(-1)["routes"] as differences, the point-wise bound the x-step is held to,
and a CDS product with one wrong seam point (numpy) that shows the bound has teeth."""
import numpy as np

from tests.sweep_geometry import _cdiv, _parts

MARCH_NT = 512          # threads of a k_cds_march workgroup (MARCH_NT)
RM_NT = 256             # threads of a k_rhs_march workgroup (RM_NT)
RM_MAXB, RM_MAXY = 8, 3     # blocks / y-difference blocks k_rhs_march takes; more: k_rhs
KERNELS = {"cds": (MARCH_NT, 2048), "rhs": (RM_NT, 4096)}       # threads, work items the default chunk count aims at
F32, F64 = "float32", "float64"


def geometry(kernel, n, TF, zchunk_env=0):
    """What march_geom (kernel "cds") / try_rhs_march ("rhs") derive for a 3-D grid n in precision TF, the march forced with
    chunks of zchunk_env planes (0: unset).  One rank: all planes."""
    NT, aim = KERNELS[kernel]
    V = 4 if np.dtype(TF) == np.float32 else 2
    n1, n2, n3 = n
    assert n1 % V == 0, "the march refuses a grid line that is no multiple of V"
    nvx = n1 // V
    lg = 0
    while (1 << lg) < nvx and lg < 6:
        lg += 1
    LX = 1 << lg
    TY = NT // LX
    tiles_x, tiles_y = _cdiv(nvx, LX), _cdiv(n2, TY)
    tiles, planes = tiles_x * tiles_y, n3
    zchunk = planes * tiles // aim
    if zchunk < 16:
        zchunk = 16
    if zchunk_env > 0:
        zchunk = zchunk_env
    if zchunk > planes:
        zchunk = planes
    nchunks = _cdiv(planes, zchunk)
    return dict(V=V, nvx=nvx, lg=lg, LX=LX, TY=TY, n2=n2, tiles_x=tiles_x, tiles_y=tiles_y, zchunk=zchunk, items=tiles * nchunks,
                tile_lanes=_parts(nvx, LX), tile_rows=_parts(n2, TY), chunks=_parts(planes, zchunk))


# ---- the properties a shape can be listed for: name -> predicate on geometry() ----------------------------------------------
PROPERTIES = {
    # the point left of a tile comes from memory (ldx1 / B.y[e0 - 1]): a tile edge inside the grid line, idle lanes in the last tile
    "two tiles along x, the last one ragged": lambda g: g["tiles_x"] >= 2 and g["tile_lanes"][-1] < g["LX"],
    # the row in front of / behind a tile comes from memory: tile edges along y inside the plane, idle rows in the last tile
    "ragged tiles_y": lambda g: g["tiles_y"] >= 2 and g["tile_rows"][-1] < g["TY"],
    # rows share a wave: the shuffles pull across rows at tx == 0 / LX - 1, and the (tid & 63) edge loads fire inside a row of threads
    "rows share a wave": lambda g: g["LX"] < 64 and min(g["TY"], g["n2"]) >= 2,
    "LX <= 2": lambda g: g["LX"] <= 2,
    # the plane has fewer rows than the tile: the row below the last one comes from memory, not from LDS
    "n2 < TY": lambda g: g["n2"] < g["TY"],
    # the plane in front of a chunk is loaded again: chunk edges inside the grid, the last chunk shorter than the others
    "three chunks, last one short": lambda g: len(g["chunks"]) >= 3 and g["chunks"][-1] < g["chunks"][0],
}

X2, TYR, WAVE, LX2, SHORT, CH3 = PROPERTIES
ALL4 = [("cds", F32), ("cds", F64), ("rhs", F32), ("rhs", F64)]


def _on(*combos_by_prop):
    """{(kernel, precision): [properties]} from (property, combos) pairs"""
    out = {c: [] for c in ALL4}
    for name, combos in combos_by_prop:
        for c in combos:
            out[c].append(name)
    return out


# shape, chunk of planes (both ZCHUNK knobs), {(kernel, precision): properties it must have}, {(kernel, precision): exact facts}
TABLE = [
    dict(n=(264, 10, 7), zchunk=3,
         props=_on((X2, ALL4), (TYR, ALL4), (CH3, ALL4)),
         facts={("cds", F32): dict(LX=64, TY=8, tile_lanes=[64, 2], tile_rows=[8, 2], chunks=[3, 3, 1]),
                ("cds", F64): dict(LX=64, TY=8, tile_lanes=[64, 64, 4], tile_rows=[8, 2]),
                ("rhs", F32): dict(LX=64, TY=4, tile_lanes=[64, 2], tile_rows=[4, 4, 2], chunks=[3, 3, 1]),
                ("rhs", F64): dict(LX=64, TY=4, tile_lanes=[64, 64, 4], tile_rows=[4, 4, 2])}),
    dict(n=(36, 40, 9), zchunk=4,
         props=_on((WAVE, ALL4), (CH3, ALL4), (TYR, [("cds", F32), ("cds", F64), ("rhs", F32)])),
         facts={("cds", F32): dict(LX=16, TY=32, tile_lanes=[9], tile_rows=[32, 8], chunks=[4, 4, 1]),
                ("cds", F64): dict(LX=32, TY=16, tile_lanes=[18], tile_rows=[16, 16, 8]),
                ("rhs", F32): dict(LX=16, TY=16, tile_lanes=[9], tile_rows=[16, 16, 8]),
                ("rhs", F64): dict(LX=32, TY=8, tile_lanes=[18], tile_rows=[8, 8, 8, 8, 8])}),
    dict(n=(4, 516, 5), zchunk=2,
         props=_on((LX2, ALL4), (WAVE, ALL4), (TYR, ALL4), (CH3, ALL4)),
         facts={("cds", F32): dict(LX=1, TY=512, tile_lanes=[1], tile_rows=[512, 4], chunks=[2, 2, 1]),
                ("cds", F64): dict(LX=2, TY=256, tile_lanes=[2], tile_rows=[256, 256, 4]),
                ("rhs", F32): dict(LX=1, TY=256, tile_lanes=[1], tile_rows=[256, 256, 4]),
                ("rhs", F64): dict(LX=2, TY=128, tile_lanes=[2], tile_rows=[128, 128, 128, 128, 4])}),
    dict(n=(132, 18, 7), zchunk=3,
         props=_on((X2, [("cds", F64), ("rhs", F64)]), (TYR, ALL4), (CH3, ALL4)),
         facts={("cds", F32): dict(LX=64, TY=8, tile_lanes=[33], tile_rows=[8, 8, 2], chunks=[3, 3, 1]),
                ("cds", F64): dict(LX=64, TY=8, tile_lanes=[64, 2], tile_rows=[8, 8, 2]),
                ("rhs", F32): dict(LX=64, TY=4, tile_lanes=[33], tile_rows=[4, 4, 4, 4, 2]),
                ("rhs", F64): dict(LX=64, TY=4, tile_lanes=[64, 2], tile_rows=[4, 4, 4, 4, 2])}),
    # a plane shorter than the tile: 32 rows of threads on 20 rows in Float32 at 512 threads ...
    dict(n=(36, 20, 9), zchunk=4,
         props=_on((SHORT, [("cds", F32)]), (WAVE, ALL4), (CH3, ALL4)),
         facts={("cds", F32): dict(LX=16, TY=32, tile_rows=[20], chunks=[4, 4, 1]),
                ("cds", F64): dict(LX=32, TY=16, tile_rows=[16, 4]),
                ("rhs", F32): dict(LX=16, TY=16, tile_rows=[16, 4]),
                ("rhs", F64): dict(LX=32, TY=8, tile_rows=[8, 8, 4])}),
    # ... and in every kernel and precision (the smallest tile, k_rhs_march in Float64, has 8 rows)
    dict(n=(36, 6, 9), zchunk=4,
         props=_on((SHORT, ALL4), (WAVE, ALL4), (CH3, ALL4)),
         facts={("cds", F32): dict(TY=32, tile_rows=[6]), ("cds", F64): dict(TY=16, tile_rows=[6]),
                ("rhs", F32): dict(TY=16, tile_rows=[6]), ("rhs", F64): dict(TY=8, tile_rows=[6], chunks=[4, 4, 1])}),
]
SEAM_X = (264, 10, 7)       # two tiles along x in both precisions and both kernels


def entry(n):
    for e in TABLE:
        if e["n"] == tuple(n):
            return e
    raise KeyError(n)


def second_tile_row(n, TF, j, k, kernel="cds"):
    """row of the first point of the second x-tile in grid row j of plane k (grid index (LX V, j, k)): its left neighbour is
    fetched from memory"""
    g = geometry(kernel, n, TF, entry(n)["zchunk"])
    assert g["tiles_x"] >= 2 and j < n[1] and k < n[2]
    return g["LX"] * g["V"] + n[0] * (j + n[1] * k)


# ---- route counters ------------------------------------------------------------------------------------------------------------
def routes(ctx):
    """launches per route since the context was finalised (kernel_stats_all(-1)["routes"])"""
    return dict(ctx.kernel_stats_all(-1)["routes"])


def ran(after, before):
    """the routes launched between two readings, with their launches"""
    return {k: v - before.get(k, 0) for k, v in after.items() if v != before.get(k, 0)}


def assert_route(took, must, never, what):
    """`took` (from ran): every name of `must` was launched; nothing whose name contains an entry of `never` was."""
    missing = [k for k in must if took.get(k, 0) <= 0]
    stray = sorted(k for k in took if any(s in k for s in never))
    assert not missing and not stray, f"{what}: the forced route was not taken: expected {must}, not launched {missing}, launched instead {stray}; all launches {took}"


FLAT_ONLY = ["k_cds_march", "k_rhs_march"]            # for `never`: substrings of route names
MARCH_ONLY = ["k_cds<", "k_cds_fused"]


# ---- the point-wise bound on the x-step ----------------------------------------------------------------------------------------
def pointwise_bound(TF, cg_it, N, x_ref, x0):
    """4 cg_it c eps max|x_ref - x0|.  Float32 (c = 1): the engine's element-wise arithmetic is the oracle's; what can differ is
    a reduction rounded to TF from a float64 sum taken in another order, at most one ulp in alpha or beta per iteration.
    Float64 (c = N): the reductions themselves are float64 sums in another order, at most N 2^-53 each."""
    c = 1 if np.dtype(TF) == np.float32 else N
    return 4.0 * cg_it * c * float(np.finfo(TF).eps) * float(np.abs(x_ref.astype(np.float64) - x0.astype(np.float64)).max())


def max_difference(a, b, shape):
    """(max |a - b|, its grid index)"""
    d = np.abs(a.astype(np.float64) - b.astype(np.float64))
    at = int(np.argmax(d))
    return float(d[at]), tuple(int(c) for c in np.unravel_index(at, shape, order="F"))


def faulty_product(Afun, Q, off, row):
    """v -> Q v with ONE wrong seam point: at `row` the left neighbour is taken from one element further left, as a tile whose
    edge load is off by one would (numpy; band -1 of the matrix: Q[row, row - 1] v[row - 2] for Q[row, row - 1] v[row - 1])"""
    b = int(np.nonzero(np.asarray(off) == -1)[0][0])

    def f(v):
        y = Afun(v, Q, off)
        acc = v.dtype.type(0)       # the row's sum again in band order, as CDS_MVp adds it, with the one wrong operand
        for i, d in enumerate(int(o) for o in off):
            if 0 <= row + d < len(v):
                acc = acc + Q[row, i] * (v[row - 2] if i == b else v[row + d])
        y[row] = acc
        return y
    return f
