"""The plain depthwise kernel instances (csrc/dwconv.hip) as a table, a pure mirror of the routing its four entry points do
(mliis_dwconv_fwd, mliis_dwconv_bwd_data, mliis_dwconv_bwd_data_bn, mliis_dwconv_bwd_filter), and the cases that reach every
instance a call below 2 GiB can launch.  Shared by test_dwconv_instances_cpu.py (the table against the source, the mirror against the
library's workspace query: host code, no GPU) and test_dwconv_instances_gpu.py (float64 parity per case).

The launchers choose among five templates -- the sliding-window dwconv_fwd_k / dwconv_fwd_stats_k / dwconv_bwd_data_k, the LDS-tile
dwconv_tile_k in its FLIP / STATS / DIL / BNB forms and dwconv_bwd_filter_k -- by k, stride, tensor size, whether statistics ride
along and how large the caller's partial buffer is.  A buffer size is therefore part of a case: the 5x5 stride-1 forward with
statistics takes the sliding-window kernel only when the buffer holds ceil(strips / 32) * 2 * C floats but not tile.blocks * 2 * C, and
mliis_dwconv_bwd_data_bn falls back to an unfused kernel (reporting 0 blocks) when `part` is short of tile.blocks * 2 * C.

This file imports neither torch nor the library: the mirror only picks shapes and predicts routes; the CPU test ties it to the
source and to mliis_dwconv_bwd_filter_workspace_floats, the GPU test to the block counts the library reports."""
import collections

TW = 4                      # kTW: outputs per strip of the sliding-window kernels
TOH, TOW, TS = 7, 16, 4     # dw_tile: 7 x 16 outputs per LDS tile, strips of 4
STATS_STRIPS = 32           # strips per workgroup of dwconv_fwd_stats_k: (strips + 31) / 32
FILTER_WANT = 512           # dw_filter_geom: want = 512 / ny blocks
LIMIT = 1 << 31             # 32-bit buffer offsets: the tile kernels take tensors below 2 GiB

KS = ((3, 1), (3, 2), (5, 1), (5, 2))     # DW_DISPATCH

# kernel: "fwd" | "fwd_stats" | "bwd_data" | "bwd_filter" (dwconv_*_k<k, s, kTW>) | "tile" (dwconv_tile_k<k, s, ...>, whose s is the
# template's S: the backward-data launches always run the stride-1 geometry and express a stride-2 LAYER as dil)
Instance = collections.namedtuple("Instance", "kernel k s flip stats dil bnb")


def sliding(kernel, k, s):
    return Instance(kernel, k, s, False, False, False, False)


def tile(k, s, flip=False, stats=False, dil=False, bnb=False):
    return Instance("tile", k, s, flip, stats, dil, bnb)


def kernel_name(i):
    """The template instance as hipcc spells it."""
    if i.kernel != "tile":
        return "dwconv_{}_k<{}, {}, {}>".format(i.kernel, i.k, i.s, TW)
    b = {True: "true", False: "false"}
    tow, ts = (TOW, TS) if i.s == 1 else (7, 1)
    return "dwconv_tile_k<{}, {}, {}, {}, {}, {}, {}, {}, {}>".format(i.k, i.s, TOH, tow, ts, b[i.flip], b[i.stats], b[i.dil], b[i.bnb])


# launch_dw_tile<FLIP, STATS, DIL, BNB> as its callers spell it: forward with and without statistics, backward-data of a stride-1 /
# stride-2 layer with and without the batch-norm sums
TILE_FORMS = ((False, True, False, False), (False, False, False, False),
              (True, False, False, True), (True, False, True, True), (True, False, False, False), (True, False, True, False))


def declared():
    """Everything the launch code can name: DW_DISPATCH gives 4 x 4 sliding-window instances; each of the six launch_dw_tile forms
    instantiates a 3x3 and a 5x5 stride-1 tile kernel and the 5x5 stride-2 one, which drops DIL and BNB (6 + 6 + 3): 31 in all."""
    out = [sliding(kern, k, s) for kern in ("fwd", "fwd_stats", "bwd_data", "bwd_filter") for k, s in KS]
    for flip, stats, dil, bnb in TILE_FORMS:
        for inst in (tile(3, 1, flip, stats, dil, bnb), tile(5, 1, flip, stats, dil, bnb), tile(5, 2, flip, stats, False, False)):
            if inst not in out:
                out.append(inst)
    return tuple(out)


INSTANCES = declared()

_BIG = ("Only a tensor of 2 GiB or more gets here: below that every 5x5 {} goes through the LDS-tile kernel, and the suite "
        "allocates no such tensor.")
_S2 = ("mliis_dwconv_fwd sends only stride-1 layers through the tile kernel (tiled requires stride == 1) and the backward-data "
       "launches always pass stride 1 to launch_dw_tile, so its stride-2 branch is never taken.")
_K3 = ("A 3x3 layer reaches launch_dw_tile only from backward-data with the batch-norm sums (small && (k == 5 || fuse)); {} "
       "never sends one there.")
# instance -> why no call below 2 GiB launches it.  The dead instantiations stay in the library for now (a follow-up removes them).
UNREACHABLE = {
    sliding("fwd", 5, 1): _BIG.format("stride-1 forward without statistics"),
    sliding("bwd_data", 5, 1): _BIG.format("backward-data launch"),
    sliding("bwd_data", 5, 2): _BIG.format("backward-data launch"),
    tile(5, 2, False, True): _S2,
    tile(5, 2, False, False): _S2,
    tile(5, 2, True, False): _S2,
    tile(3, 1, False, True): _K3.format("the forward tiles 5x5 layers only, so the statistics form"),
    tile(3, 1, False, False): _K3.format("the forward tiles 5x5 layers only, so the plain form"),
    tile(3, 1, True, False, False, False): _K3.format("without the sums a 3x3 stride-1 layer takes dwconv_bwd_data_k, so the unfused form"),
    tile(3, 1, True, False, True, False): _K3.format("without the sums a 3x3 stride-2 layer takes dwconv_bwd_data_k, so the unfused form"),
}


# ---------------------------------------------------------------------------------------------------------------- routing mirror
def cdiv(a, b):
    return -(-a // b)


def same_pad(H, W, k, s):
    """dw_geom: (Ho, Wo, pt, pl) of TF-SAME padding."""
    Ho, Wo = cdiv(H, s), cdiv(W, s)
    return Ho, Wo, max((Ho - 1) * s + k - H, 0) // 2, max((Wo - 1) * s + k - W, 0) // 2


Tile = collections.namedtuple("Tile", "tiles_y tiles_x blocks")


def tile_geom(N, Ho, Wo):
    """dw_tile at stride 1 (the only geometry a reachable launch uses)."""
    ty, tx = cdiv(Ho, TOH), cdiv(Wo, TOW)
    return Tile(ty, tx, N * ty * tx)


def strips_of(N, Ho, Wo):
    return N * Ho * cdiv(Wo, TW)


def stats_blocks(N, H, W, k, s):
    """Blocks (= rows [2][C] of the statistics buffer) of dwconv_fwd_stats_k."""
    Ho, Wo, _, _ = same_pad(H, W, k, s)
    return cdiv(strips_of(N, Ho, Wo), STATS_STRIPS)


def fwd_route(N, H, W, C, k, s, stats_floats):
    """mliis_dwconv_fwd: (instance launched, statistics blocks reported).  stats_floats None = no statistics."""
    Ho, Wo, _, _ = same_pad(H, W, k, s)
    t = tile_geom(N, Ho, Wo)
    tiled = k == 5 and s == 1 and N * H * W * C * 4 < LIMIT and t.blocks < LIMIT
    if stats_floats is not None:
        nblk = cdiv(strips_of(N, Ho, Wo), STATS_STRIPS)
        if nblk * 2 * C > stats_floats:
            raise ValueError("statistics buffer too small: {} floats needed, {} given".format(nblk * 2 * C, stats_floats))
        if tiled and t.blocks * 2 * C <= stats_floats:
            return tile(5, 1, False, True), t.blocks
        return sliding("fwd_stats", k, s), nblk
    if tiled:
        return tile(5, 1), 0
    return sliding("fwd", k, s), 0


def bwd_data_route(N, H, W, C, k, s, with_bn, part_floats):
    """dw_bwd_data: (instance launched, stage-1 blocks reported); the tiles cover the layer's INPUT.  0 blocks = "not produced"."""
    t = tile_geom(N, H, W)
    small = N * H * W * C * 4 < LIMIT and t.blocks < LIMIT
    fuse = bool(with_bn) and small and t.blocks * 2 * C <= part_floats
    if small and (k == 5 or fuse):
        return tile(k, 1, True, False, s == 2, fuse), (t.blocks if fuse else 0)
    return sliding("bwd_data", k, s), 0


FilterGeom = collections.namedtuple("FilterGeom", "QB RP ny items items_per_block nblk idle_lanes last_group_quads last_block_items max_walk")


def filter_geom(N, H, W, C, k, s):
    """dw_filter_geom, and what follows from it for dwconv_bwd_filter_k: lanes of the 256 that own no (quad, strip-lane) pair, quads
    in the last channel group, strips left for the last block, and the most iterations any thread's walk `it += RP` makes."""
    Ho, Wo, _, _ = same_pad(H, W, k, s)
    Q = C // 4
    QB = min(Q, 64)
    RP = 256 // QB
    ny = cdiv(Q, QB)
    items = strips_of(N, Ho, Wo)
    want = max(FILTER_WANT // ny, 1)
    ipb = cdiv(max(cdiv(items, want), RP), RP) * RP
    nblk = cdiv(items, ipb)
    return FilterGeom(QB, RP, ny, items, ipb, nblk, 256 - QB * RP, Q - (ny - 1) * QB, items - (nblk - 1) * ipb, cdiv(min(ipb, items), RP))


# ---------------------------------------------------------------------------------------------------------------- cases
# (N, H, W, C) of the layer's INPUT.
RAGGED = (2, 15, 33, 40)     # stride 1: 3 x 3 tiles with Ho % 7, Wo % 16 and Wo % 4 tails, channel groups 32 + 8, 270 strips -> 9 statistics
#                              blocks (14 live lanes in the last) against 18 tile blocks; stride 2: 8 x 17 outputs
TINY = ((1, 1, 1, 4), (3, 2, 3, 12))     # maps smaller than the filter: every tap but the centre ones is padding; one and three quads
TINY_GAP = (2, 1, 1, 4)      # stands in for TINY[0] where the route needs ceil(strips/32) < tile.blocks: one image has one block of each
EVEN, MIXED = (2, 16, 34, 40), (2, 16, 33, 40)     # stride 2: pt = pl, and H even / W odd: k = 3 -> pt 0, pl 1; k = 5 -> pt 1, pl 2
GROUPS = (2, 15, 33, 288)    # filter gradient: two channel groups, 8 of 64 quads in the last; stride 1: last block 2 of 4 strips
GROUPS_S2 = (2, 13, 33, 288)     # the same with a partial last block at stride 2 (70 strips = 17 blocks of 4 + 2)
WALK = {1: (2, 33, 66, 288), 2: (2, 66, 132, 288)}     # 1122 strips, 8 per block: every thread walks twice, the last block holds 2

# kind: ragged | tiny | even | mixed | fallback (bwd_data_bn) | idle | groups | walk (bwd_filter).  k, s: the LAYER's.  floats: the
# size of the statistics / stage-1 buffer handed to the call (None: the call takes none), or the filter workspace's extent.
Case = collections.namedtuple("Case", "inst kind shape k s floats")

ENTRY_OF = {"fwd": "fwd", "fwd_stats": "fwd", "bwd_data": "bwd_data", "bwd_filter": "bwd_filter"}


def layer_of(i):
    """(k, stride) of the layer an instance serves."""
    return i.k, (2 if i.dil else i.s)


def entry_of(c):
    """Which entry point a case calls: fwd | bwd_data | bwd_data_bn | bwd_filter."""
    i = c.inst
    if i.kernel != "tile":
        return ENTRY_OF[i.kernel]
    return "fwd" if not i.flip else ("bwd_data_bn" if i.bnb else "bwd_data")


def launched(c):
    """(instance, nblk) the mirror says the case's call launches: c.inst itself but for a fallback case, which belongs to a BNB
    instance and runs what mliis_dwconv_bwd_data_bn substitutes for it."""
    N, H, W, C = c.shape
    e = entry_of(c)
    if e == "fwd":
        return fwd_route(N, H, W, C, c.k, c.s, c.floats)
    if e == "bwd_filter":
        return c.inst, filter_geom(N, H, W, C, c.k, c.s).nblk
    return bwd_data_route(N, H, W, C, c.k, c.s, e == "bwd_data_bn", c.floats or 0)


def _shapes(s, tiny0=TINY[0]):
    out = [("ragged", RAGGED), ("tiny", tiny0), ("tiny", TINY[1])]
    if s == 2:
        out += [("even", EVEN), ("mixed", MIXED)]
    return out


def cases():
    out = []
    for i in INSTANCES:
        if i in UNREACHABLE:
            continue
        k, s = layer_of(i)
        if i.kernel == "bwd_filter":
            shapes = [("idle", RAGGED), ("idle", TINY[1]), ("groups", GROUPS), ("walk", WALK[s])] + ([("groups", GROUPS_S2)] if s == 2 else [])
            for kind, shape in shapes:
                out.append(Case(i, kind, shape, k, s, filter_geom(*shape, k, s).nblk * k * k * shape[3]))
            continue
        gap = i == sliding("fwd_stats", 5, 1)      # reached only through a buffer too small for the tile layout
        for kind, shape in _shapes(s, TINY_GAP if gap else TINY[0]):
            N, H, W, C = shape
            Ho, Wo, _, _ = same_pad(H, W, k, s)
            floats = None
            if i.kernel == "fwd_stats":            # the boundary: exactly its own layout, or one float short of the tile layout
                floats = tile_geom(N, Ho, Wo).blocks * 2 * C - 1 if gap else stats_blocks(N, H, W, k, s) * 2 * C
            elif i.stats:
                floats = tile_geom(N, Ho, Wo).blocks * 2 * C
            elif i.bnb:
                floats = tile_geom(N, H, W).blocks * 2 * C
            out.append(Case(i, kind, shape, k, s, floats))
            if i.bnb and kind in ("ragged", "mixed"):
                out.append(Case(i, "fallback", shape, k, s, floats - 1))
    return out


def short_name(i):
    if i.kernel != "tile":
        return "{}-k{}s{}".format(i.kernel, i.k, i.s)
    flags = "".join(n for n, on in (("-flip", i.flip), ("-stats", i.stats), ("-dil", i.dil), ("-bnb", i.bnb)) if on)
    return "tile-k{}s{}{}".format(i.k, i.s, flags)


def case_id(c):
    return "{}-{}-{}{}".format(short_name(c.inst), c.kind, "x".join(map(str, c.shape)), "" if c.floats is None else "-f{}".format(c.floats))
