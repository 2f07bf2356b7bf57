"""The launch geometry of the one-sweep y/l update, restated (pure Python, no GPU).

`geometry` follows launch_multi of csrc/kernels_multi.hip line by line: points per thread, the tile of LX lanes by TY
rows, the tiles of a plane, the segments of a 2-D grid line (xsplit) and the chunks of planes.  TABLE lists the small
grids the seam tests run on, each with the properties it is there for; tests/test_gpu_sweep_geometry.py proves every
listed property on the CPU, so a change of a tile constant fails there instead of silently moving a seam off the grid."""
import numpy as np

MULTI_NT = 256          # threads of a workgroup (MULTI_NT)
MULTI_VF = 4            # points per thread in Float32 (SIPX_MULTI_VF); Float64: half as many
NB_7 = 1792             # workgroup slots the chunk count aims at (csrc/sipx_common.h)


def _cdiv(a, b):
    return -(-a // b)


def _parts(total, piece):
    """total cut into pieces of `piece`, the last one shorter: [piece, ..., rest]"""
    return [min(piece, total - k) for k in range(0, total, piece)]


def geometry(n, TF, zchunk_env=0):
    """What launch_multi derives for a grid n = (n1, n2) or (n1, n2, n3) in precision TF with SIPX_MULTI_ZCHUNK = zchunk_env
    (0: unset).  One rank: rows [0, n2) of every plane, planes [0, n_last)."""
    V = MULTI_VF if np.dtype(TF) == np.float32 else MULTI_VF // 2
    n1 = n[0]
    assert n1 % V == 0, "yl_multi refuses a grid line that is no multiple of V"
    nvx = n1 // V
    lg = 0
    while (1 << lg) < nvx and lg < 6:
        lg += 1
    LX = 1 << lg
    TY = MULTI_NT // LX
    three = len(n) == 3 and n[1] > 1                 # a 2-D grid arrives as (n1, 1, n2): marched along its second dimension
    xsplit = not three
    rows = n[1] if three else 1
    planes = n[-1]
    tiles_x = _cdiv(nvx, LX * TY) if xsplit else _cdiv(nvx, LX)
    tiles_y = 1 if xsplit else _cdiv(rows, TY)
    tiles = tiles_x * tiles_y
    want = max(1, _cdiv(4 * NB_7, tiles))
    zchunk = _cdiv(planes, want)
    if zchunk < 8:
        zchunk = min(planes, 8)
    if zchunk_env > 0:
        zchunk = min(zchunk_env, planes)
    g = dict(V=V, nvx=nvx, lg=lg, LX=LX, TY=TY, xsplit=xsplit, tiles_x=tiles_x, tiles_y=tiles_y, zchunk=zchunk,
             chunks=_parts(planes, zchunk))
    # lanes (threads along x that own points) of every tile along x; xsplit: a tile holds TY segments of LX lanes
    g["tile_lanes"] = _parts(nvx, LX * TY if xsplit else LX)
    g["tile_rows"] = [1] if xsplit else _parts(rows, TY)
    # xsplit: lanes of every active segment, per tile
    g["segments"] = [_parts(t, LX) for t in g["tile_lanes"]] if xsplit else [[t] for t in g["tile_lanes"]]
    return g


# ---- the properties a shape can be listed for: name -> predicate on geometry() ---------------------------------------------
PROPERTIES = {
    # the point left of a tile is recomputed: there is a tile edge inside the grid line
    "two tiles along x": lambda g: g["tiles_x"] >= 2,
    # ... and the last tile has idle lanes
    "last tile ragged": lambda g: g["tile_lanes"][-1] < (g["LX"] * g["TY"] if g["xsplit"] else g["LX"]),
    # xsplit: the recomputed left point also sits at the first lane of a segment INSIDE a tile
    "two segments in one tile": lambda g: g["xsplit"] and max(len(s) for s in g["segments"]) >= 2,
    "last segment ragged": lambda g: g["xsplit"] and g["segments"][-1][-1] < g["LX"],
    # several thread rows share a wave: the shuffle that fetches the lane to the left pulls from the row above at tx == 0
    "rows share a wave": lambda g: g["LX"] < 64 and not g["xsplit"] and max(g["tile_rows"]) >= 2,
    "LX <= 2": lambda g: g["LX"] <= 2,
    # the plane in front of a chunk is recomputed: chunk edges inside the grid, the last chunk shorter than the others
    "three chunks, last one short": lambda g: len(g["chunks"]) >= 3 and g["chunks"][-1] < g["chunks"][0],
    # the row in front of a tile is recomputed: tile edges along y inside the plane, the last tile with idle rows
    "ragged tiles_y": lambda g: g["tiles_y"] >= 2 and g["tile_rows"][-1] < g["TY"],
}

F32, F64 = "float32", "float64"

# (shape, spacings, SIPX_MULTI_ZCHUNK or 0, properties both precisions must have, {precision: exact facts of geometry()})
TABLE = [
    dict(n=(264, 10, 7), h=(25.0, 20.0, 10.0), zchunk=3,
         props=["two tiles along x", "last tile ragged", "ragged tiles_y", "three chunks, last one short"],
         facts={F32: dict(LX=64, TY=4, tile_lanes=[64, 2], tile_rows=[4, 4, 2], chunks=[3, 3, 1]),
                F64: dict(LX=64, TY=4, tile_lanes=[64, 64, 4], tile_rows=[4, 4, 2], chunks=[3, 3, 1])}),
    dict(n=(4, 260, 5), h=(25.0, 20.0, 10.0), zchunk=0,
         props=["LX <= 2", "rows share a wave", "ragged tiles_y"],
         facts={F32: dict(LX=1, TY=256, tile_lanes=[1], tile_rows=[256, 4], chunks=[5]),
                F64: dict(LX=2, TY=128, tile_lanes=[2], tile_rows=[128, 128, 4], chunks=[5])}),
    dict(n=(36, 20, 9), h=(25.0, 20.0, 10.0), zchunk=4,
         props=["rows share a wave", "last tile ragged", "ragged tiles_y", "three chunks, last one short"],
         facts={F32: dict(LX=16, TY=16, tile_lanes=[9], tile_rows=[16, 4], chunks=[4, 4, 1]),
                F64: dict(LX=32, TY=8, tile_lanes=[18], tile_rows=[8, 8, 4], chunks=[4, 4, 1])}),
    dict(n=(1304, 11), h=(25.0, 6.0), zchunk=4,
         props=["two tiles along x", "last tile ragged", "two segments in one tile", "last segment ragged", "three chunks, last one short"],
         facts={F32: dict(LX=64, TY=4, tile_lanes=[256, 70], segments=[[64] * 4, [64, 6]], chunks=[4, 4, 3]),
                F64: dict(LX=64, TY=4, tile_lanes=[256, 256, 140], segments=[[64] * 4, [64] * 4, [64, 64, 12]], chunks=[4, 4, 3])}),
    dict(n=(264, 9), h=(25.0, 6.0), zchunk=0,
         props=["two segments in one tile", "last segment ragged", "last tile ragged"],
         facts={F32: dict(LX=64, TY=4, tiles_x=1, segments=[[64, 2]], chunks=[8, 1]),
                F64: dict(LX=64, TY=4, tiles_x=1, segments=[[64, 64, 4]], chunks=[8, 1])}),
    dict(n=(4, 40), h=(25.0, 6.0), zchunk=0,
         props=["LX <= 2"],
         facts={F32: dict(LX=1, TY=256, tiles_x=1, segments=[[1]], chunks=[8] * 5),
                F64: dict(LX=2, TY=128, tiles_x=1, segments=[[2]], chunks=[8] * 5)}),
]


def entry(n):
    for e in TABLE:
        if e["n"] == tuple(n):
            return e
    raise KeyError(n)
