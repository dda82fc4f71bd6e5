"""The split-product kernel instances (csrc/conv_x3.hip) as a manifest, a Python mirror of their planner, the stream-K cut geometry
derived from it, and a search for the cheapest shapes that launch each instance.  No device work: the library's planner queries answer
without a GPU (the CU count falls back to the MI355X's 256).

conv_x3_k<NT> / x3_fixup_k<NT> (NT = 1..9) and conv_filter_x3_batched_k<NT> (NT = 4..8, three bodies) are separately compiled code:
pieces per thread, the placement of the in-flight split, the fragment ring and the fix-up's lane layout all depend on NT.  declared() is
what the launch switches name, search() / search_filter() what the planners pick, UNREACHABLE why the rest cannot be picked;
test_x3_instances_cpu.py holds the three together and test_x3_instances_gpu.py launches every reached instance (conv_instances.py
does the same for the fp32 / bf16 / fp8 kernels).

A conv shape is (N, H, W, Cred, Nout, ksize, dil): Cred channels are reduced per tap, Nout columns come out.  Forward: Cred = Cin,
Nout = Cout; backward-data: Cred = Cout, Nout = Cin -- the same GEMM with the taps mirrored (sign = -1)."""
import collections
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SOURCE = os.path.join(ROOT, "mliis_amd", "csrc", "conv_x3.hip")

# ---------------------------------------------------------------------------------------------------------------- declared instances
X3_NT = tuple(range(1, 10))          # x3_launch: conv_x3_k<NT> + x3_fixup_k<NT>
FILTER_NT = tuple(range(4, 9))       # launch_filter_batched_x3: conv_filter_x3_batched_k<NT>
FILTER_BODIES = ("128", "256", "multitap")   # conv_filter_x3_body<NT, 128 | 256>; multitap: a run-time branch of the 128 body with its own indexing
DIRECTIONS = ("fwd", "bwd")          # sign = +1 | -1 of the same instantiation


def conv_name(nt, direction):
    return "conv_x3_k<{}> {}".format(nt, direction)


def fixup_name(nt):
    return "x3_fixup_k<{}>".format(nt)


def filter_name(nt, body):
    return "conv_filter_x3_batched_k<{}> {}".format(nt, body)


def declared():
    return ({conv_name(nt, d) for nt in X3_NT for d in DIRECTIONS} | {fixup_name(nt) for nt in X3_NT} |
            {filter_name(nt, b) for nt in FILTER_NT for b in FILTER_BODIES})


def parse_switches(path=SOURCE):
    """(conv NTs, the kernels one conv case launches, filter NTs, filter body widths) as the two launch switches and the batched
    kernel's body dispatch spell them."""
    src = open(path).read()

    def body(signature):
        i = src.index(signature)
        return src[i:src.index("#undef L", i)]

    conv = body("static void x3_launch(")
    kernels = tuple(re.findall(r"hipLaunchKernelGGL\(\((\w+)<NT_>\)", conv))
    conv_nt = tuple(int(v) for v in re.findall(r"(?:case \d+|default): L\((\d+)\)", conv))
    assert [int(v) for v in re.findall(r"case (\d+): L\(", conv)] == list(conv_nt[:-1]), "a case label launches another width"
    filt = body("bool launch_filter_batched_x3(")
    filt_nt = tuple(int(v) for v in re.findall(r"case \d+: L\((\d+)\)", filt))
    assert [int(v) for v in re.findall(r"case (\d+): L\(", filt)] == list(filt_nt)
    widths = tuple(sorted({int(v) for v in re.findall(r"conv_filter_x3_body<NT, (\d+)>\(", src)}))
    return conv_nt, kernels, filt_nt, widths


# declared instance -> the planner line that keeps every call away from it.  Empty: x3_pick_nt names every width 1..9 and x3_plan's
# narrowing only ever leaves a width of the list; plan_filter names every column-tile count 4..8 with TMF = 2, multitap or not.
UNREACHABLE = {}

# ---------------------------------------------------------------------------------------------------------------- planner mirror
NUM_CUS = 256
BM = 256            # kX3BM
MIN_PART = 4        # kX3MinPart
MAX_NT = 9          # kX3MaxNT
FIX = 4             # kX3Fix

Plan = collections.namedtuple("Plan", "nt gx gy nchunks parts ipp smax")
Shape = collections.namedtuple("Shape", "N H W Cred Nout ksize dil")


def rows(s):
    return s.N * s.H * s.W


def kred(s):
    return s.ksize * s.ksize * s.Cred


def cost(s):
    return rows(s) * kred(s) * s.Nout


def pick_nt(nout):
    """x3_pick_nt: the same double arithmetic in the same order."""
    best, best_cost = 1, 1e30
    tiles = (nout + 15) // 16
    for nt in range(1, MAX_NT + 1):
        blocks = (tiles + nt - 1) // nt
        c = float(blocks * nt * 16) / float(nout) * (1.0 + 0.08 * (8 - nt))
        if c < best_cost - 1e-9 or (c < best_cost + 1e-9 and nt > best):
            best_cost, best = c, nt
    return best


def chunks(ntaps, cred):
    return (ntaps * cred + 31) // 32


def plan(M, nout, ntaps, cred, cus=NUM_CUS):
    """x3_plan."""
    nt = pick_nt(nout)
    gy = (nout + nt * 16 - 1) // (nt * 16)
    gx = (M + BM - 1) // BM
    nch = chunks(ntaps, cred)
    while nt > 2 and gx * gy * nch < cus * 2 * MIN_PART:
        nt = (nt + 1) // 2
        gy = (nout + nt * 16 - 1) // (nt * 16)
    tiles = gx * gy
    total = tiles * nch
    parts = min(cus, 8 * tiles)
    if total // parts < MIN_PART:
        parts = total // MIN_PART
    parts = max(parts, 1)
    ipp = (total + parts - 1) // parts
    return Plan(nt, gx, gy, nch, (total + ipp - 1) // ipp, ipp, (nch + ipp - 1) // ipp + 1)


def plan_of(s, cus=NUM_CUS):
    return plan(rows(s), s.Nout, s.ksize * s.ksize, s.Cred, cus)


def workspace_floats(p):
    return p.gx * p.gy * p.smax * BM * 16 * p.nt


def lib_plan(s):
    """(nt, gx, gy, full, parts, ipp, smax, nchunks) of mliis_conv2d_x3_plan."""
    import ctypes as C
    from mliis_amd._lib import lib
    out = (C.c_int * 8)()
    lib.call("mliis_conv2d_x3_plan", s.N, s.H, s.W, s.Cred, s.Nout, s.ksize, C.cast(out, C.c_void_p))
    return tuple(out)


def lib_workspace_floats(s):
    from mliis_amd._lib import lib
    return lib.size("mliis_conv2d_x3_workspace_floats", s.N, s.H, s.W, s.Cred, s.Nout, s.ksize)


# ---------------------------------------------------------------------------------------------------------------- cut geometry
def segments(p):
    """[(part, tile, c0, c1)]: the K-chunk ranges conv_x3_k's workgroups walk, in their order."""
    out, total = [], p.gx * p.gy * p.nchunks
    for part in range(p.parts):
        lo, hi = part * p.ipp, min((part + 1) * p.ipp, total)
        while lo < hi:
            rt = lo // p.nchunks
            c0 = lo - rt * p.nchunks
            c1 = min(c0 + hi - lo, p.nchunks)
            out.append((part, rt, c0, c1))
            lo += c1 - c0
    return out


def slots(p):
    """Slabs x3_fixup_k folds per tile, and -- from conv_x3_k's side -- the slot every segment is written to."""
    n = []
    for rt in range(p.gx * p.gy):
        first = (rt * p.nchunks) // p.ipp
        last = min(((rt + 1) * p.nchunks - 1) // p.ipp, p.parts - 1)
        n.append(last - first + 1)
    return n


def written_slots(p):
    """tile -> sorted slots its segments land in (part - first part of the tile)."""
    w = collections.defaultdict(list)
    for part, rt, _, _ in segments(p):
        w[rt].append(part - (rt * p.nchunks) // p.ipp)
    return w


CUT_CLASSES = ("a", "b", "c1", "c2", "c3", "d1", "d2", "e", "f", "g1", "g2", "h", "i", "j", "k1", "k2", "k3", "l", "m")


def cut_classes(s):
    """The classes of stream-K cut (CUT_CLASSES; what each letter means: the conditions below) that a call of this shape produces, in
    either direction: the plan does not know the sign.
    (m) is this file's own: a tile whose first chunk is the LAST chunk of a part -- the one place where `first` of conv_x3_k, a floor
    of rt * nchunks / ipp, sits right below a step."""
    p = plan_of(s)
    segs = segments(p)
    total = p.gx * p.gy * p.nchunks
    taps, K = s.ksize * s.ksize, kred(s)
    per_part = collections.Counter(part for part, _, _, _ in segs)
    lens = {c1 - c0 for _, _, c0, c1 in segs}
    nsl = slots(p)
    out = set()
    if p.parts == 1 and total < 8:
        out.add("a")
    if max(per_part.values()) >= 3:
        out.add("b")
    out |= {"c%d" % n for n in (1, 2, 3) if n in lens}
    if any((c0 * 32) % s.Cred != 0 for _, _, c0, _ in segs):
        out.add("d1")
    if taps > 1 and s.Cred % 32 != 0 and any((32 * j) // s.Cred != (32 * j + 31) // s.Cred and (32 * j + 31) // s.Cred < taps for j in range(p.nchunks)):
        out.add("d2")
    if s.Cred == 32 and taps > 1:
        out.add("e")
    if total % p.ipp != 0:
        out.add("f")
    if p.smax in nsl:
        out.add("g1")
    if 1 in nsl:
        out.add("g2")
    if K % 32 != 0:
        out.add("h")
    if rows(s) < 16:
        out.add("i")
    if ((s.Nout + 15) // 16) % p.nt != 0:
        out.add("j")
    if s.ksize == 3 and s.dil >= s.H and s.dil >= s.W:
        out.add("k1")
    if s.ksize == 3 and s.H == 1:
        out.add("k2")
    if s.ksize == 3 and s.W == 1:
        out.add("k3")
    if any(((part + 1) * p.ipp) % p.nchunks == 0 for part in range(p.parts - 1)):
        out.add("l")
    if any((rt * p.nchunks) % p.ipp == p.ipp - 1 for rt in range(1, p.gx * p.gy)) and p.ipp > 1:
        out.add("m")
    return out


# The cheap shapes that carry the cut classes: NT <= 2 is never narrowed, so K can be as short as the contract allows.
CUT_CASES = (
    Shape(1, 3, 4, 36, 8, 1, 1),       # (a) one part of two chunks, (i), K % 32 = 4
    Shape(1, 3, 5, 40, 12, 3, 7),      # (a)-sized neighbour with nine taps: dilation beyond both sides of the map, only the centre tap is inside
    Shape(3, 20, 17, 64, 12, 1, 1),    # (b) nchunks = 2, ipp = 4: parts over two and three tiles, (l)
    Shape(3, 20, 17, 32, 40, 1, 1),    # (b) nchunks = 1: four tiles per part, gy = 2 after the narrowing to NT = 2
    Shape(4, 16, 16, 96, 16, 1, 1),    # (m) nchunks = 3, ipp = 4: tile 1 starts on the last chunk of part 0; segments of 1, 2 and 3 chunks
    Shape(1, 9, 7, 32, 20, 3, 1),      # (e) Cred == 32: the tap advances on every chunk
    Shape(1, 9, 7, 32, 20, 3, 2),
    Shape(1, 5, 9, 36, 24, 3, 1),      # (d) Cred % 32 = 4: every chunk but the first starts inside a tap, most straddle a boundary; (h)
    Shape(2, 11, 13, 44, 28, 3, 2),    # (d) two row tiles, the second with 30 rows: waves without a valid row
    Shape(1, 1, 19, 52, 20, 3, 1),     # (k) H == 1
    Shape(1, 21, 1, 52, 20, 3, 1),     # (k) W == 1
    Shape(1, 3, 2, 68, 36, 3, 3),      # (k) dil >= H and dil >= W, NT = 2 over three 16-column tiles: (j)
    Shape(2, 4, 4, 48, 16, 3, 4),      # (k) dil == H == W, two images
    Shape(1, 13, 20, 100, 24, 3, 2),   # (f) a short last part; (g) tiles folded from smax slots
)


def cut_table():
    return {s: cut_classes(s) for s in all_conv_shapes()}


# ---------------------------------------------------------------------------------------------------------------- shape search
MAX_COST = 6 * 10 ** 8   # multiply-adds M * K * Nout of the largest conv shape a search may keep (the float64 reference runs on the host)
KINDS = ("edge", "loop")

# edge: fewer than 16 rows, or a few rows more than one row tile; none square
EDGE_MAPS = {"fwd": ((1, 3, 5), (1, 2, 7), (1, 9, 29), (1, 7, 37)), "bwd": ((1, 5, 3), (1, 7, 2), (1, 29, 9), (1, 37, 7))}
# loop: two or three row tiles; forward prefers whole tiles (M % 256 == 0), backward-data a ragged last one
# (the 65-row maps: a width that is never the result of a narrowing needs 2048 chunks over its tiles, and two row tiles of such
#  chunks are beyond MAX_COST from NT = 6 on -- those loop shapes have one row tile, three or four of whose waves have valid rows)
LOOP_MAPS = {"fwd": ((2, 16, 16), (1, 16, 32), (3, 16, 16), (1, 7, 37), (1, 13, 20), (1, 5, 13)),
             "bwd": ((1, 9, 29), (1, 20, 13), (1, 17, 31), (1, 37, 7), (1, 13, 5))}


def _cred_for(nch, taps, edge):
    """The smallest contract-conforming Cred whose reduction has at least nch chunks (edge: Cred % 8 == 4)."""
    c = max((32 * (nch - 1)) // taps + 1, 32)
    c = (c + 3) // 4 * 4
    if edge and c % 8 != 4:
        c += 4
    return c


def edge_missing(s, p):
    """The promised tails an edge shape lacks."""
    return [name for name, ok in (("rows", 1 <= rows(s) % BM <= 15), ("cred", s.Cred % 8 == 4), ("cols", s.Nout % 16 != 0),
                                  ("3x3 non-square", s.ksize == 3 and s.H != s.W and min(s.H, s.W) > 1),
                                  ("narrow last tile", ((s.Nout + 15) // 16) % p.nt != 0)) if not ok]


def loop_missing(s, p, direction):
    first = {}
    for part, _, c0, c1 in segments(p):
        first.setdefault(part, c1 - c0)
    return [name for name, ok in (("first segments >= 5", min(first.values()) >= 5), ("two row tiles", p.gx >= 2), ("two column tiles", p.gy >= 2),
                                  ("whole row tiles" if direction == "fwd" else "ragged row tile", (rows(s) % BM == 0) == (direction == "fwd"))) if not ok]


# What the cost cap keeps a kind from having, and why.  (M K Nout of a width that no narrowing produces is about rows-per-tile x columns-
# per-tile x 32 x 2048 chunks whatever the tile counts: 2.7e8 x NT with whole 256-row tiles.)
EDGE_SHORTFALL = {1: {"narrow last tile"}}   # x3_pick_nt gives NT = 1 to Nout <= 16 only and the narrowing never goes below 2: one column tile


def loop_shortfall(nt, direction):
    """What a loop shape of this width and direction lacks.  Every loop shape the search returns is a 1x1 conv (the cheapest way to a
    long reduction) and every edge shape a 3x3 one; the loop shapes from NT = 6 on have 65 rows, so only three of the eight waves own a
    valid row there.  A full 256-row tile for the widths that no other test runs with one (6 and 8) costs 1.4e9 and 1.9e9 multiply-adds:
    FULL_TILE_CASES, beyond MAX_COST on purpose."""
    out = set()
    if nt == 1:
        out.add("two column tiles")          # (as above)
    if nt >= 6:
        out.add("two row tiles")             # 259 rows x 2048 / 4 chunks x 16 NT + 4 columns: 7.0e8 at NT = 6
    if direction == "fwd" and nt >= 4:
        out.add("whole row tiles")           # 512 rows instead of 259: 8.2e8 at NT = 4
    return out


def _candidates(maps, edge):
    for N, H, W in maps:
        gx = (N * H * W + BM - 1) // BM
        for nout in range(4, 300, 4):
            chain = [pick_nt(nout)]
            while chain[-1] > 2:
                chain.append((chain[-1] + 1) // 2)
            for k in (3, 1):
                want = {1, 40, 41, 45, 48, 64, 80, 96, 120, 128, 160, 256}
                for nt in chain:   # the shortest reductions at which the narrowing loop stops at this width
                    gy = (nout + nt * 16 - 1) // (nt * 16)
                    t = -(-NUM_CUS * 2 * MIN_PART // (gx * gy))
                    want |= {t + b for b in range(8)}
                for nch in sorted(want):
                    yield N, H, W, _cred_for(nch, k * k, edge), nout, k


def search():
    """(NT, direction, kind) -> the cheapest shape of that kind that launches conv_x3_k<NT> (fewest missing properties first), found
    through the mirror; test_x3_instances_cpu.py confirms every one with the library's own queries."""
    found = {}
    for direction in DIRECTIONS:
        for kind, maps in (("edge", EDGE_MAPS[direction]), ("loop", LOOP_MAPS[direction])):
            for N, H, W, cred, nout, k in _candidates(maps, kind == "edge"):
                p = plan(N * H * W, nout, k * k, cred)
                s = Shape(N, H, W, cred, nout, k, 1 + p.nt % 2 if k == 3 else 1)
                if cost(s) > MAX_COST:
                    continue
                miss = edge_missing(s, p) if kind == "edge" else loop_missing(s, p, direction)
                key = (p.nt, direction, kind)
                rank = (len(miss), cost(s), s)
                if key not in found or rank < found[key][0]:
                    found[key] = (rank, s)
    return {key: s for key, (_, s) in found.items()}


# One whole row tile (all eight waves, every row valid) of a 3x3 conv for the widths whose searched shapes have 65 rows at most and that
# the 8 x 56 x 56 cases of test_x3_gpu.py (NT 7 and 9) do not launch: 2049 chunks keep NT = 6 and 8 from being narrowed.
FULL_TILE_COST = 2 * 10 ** 9
FULL_TILE_CASES = (Shape(1, 16, 16, 7284, 84, 3, 1), Shape(1, 16, 16, 7284, 116, 3, 2))

_SEARCH = None


def searched():
    global _SEARCH
    if _SEARCH is None:
        _SEARCH = search()
    return _SEARCH


def all_conv_shapes():
    """Every conv shape the GPU file launches: the searched ones and the cut cases (both directions run each cut case)."""
    out = []
    for s in list(searched().values()) + list(CUT_CASES) + list(FULL_TILE_CASES):
        if s not in out:
            out.append(s)
    return out


def reached_conv():
    """instance name -> shapes."""
    out = collections.defaultdict(list)
    for (nt, direction, _), s in sorted(searched().items()):
        out[conv_name(nt, direction)].append(s)
        out[fixup_name(nt)].append(s)
    return out


# ---------------------------------------------------------------------------------------------------------------- filter gradients
FShape = collections.namedtuple("FShape", "N H W Cin Cout ksize dil wide")
FILTER_MAX_COST = 10 ** 9


def fcost(s):
    return s.N * s.H * s.W * s.ksize * s.ksize * s.Cin * s.Cout


def filter_plan(s):
    """(TMF, NT, multitap, gx, gy, gz, rows_per_split) of mliis_conv2d_bwd_filter_plan."""
    import ctypes as C
    from mliis_amd._lib import lib
    out = (C.c_int * 8)()
    lib.call("mliis_conv2d_bwd_filter_plan", s.N, s.H, s.W, s.Cin, s.Cout, s.ksize, C.cast(out, C.c_void_p))
    return tuple(out)[:7]


def filter_instance(s):
    """The conv_filter_x3_batched_k instance FilterBatch.launch("fp32x3") runs this problem on, or None (the native instruction):
    mliis_conv2d_bwd_filter_batched takes the groups with TMF = 2 and 4..8 column tiles; the 256-channel body serves the problems
    with more than 128 input channels of a table built with X3_WIDE."""
    tmf, nt, mt = filter_plan(s)[:3]
    if tmf != 2 or nt not in FILTER_NT:
        return None
    return filter_name(nt, "multitap" if mt else ("256" if s.wide and s.Cin > 128 else "128"))


# maps: rows that are and are not multiples of the 32-pixel chunk, one smaller than a chunk, one with several slabs
FILTER_MAPS = ((1, 5, 5), (3, 19, 21), (1, 61, 61), (4, 30, 30), (1, 91, 91))
FILTER_MULTITAP_MAPS = ((1, 129, 131), (1, 181, 183), (1, 257, 257))   # (the multitap form has one block along x: only slabs fill the chip)
# TMF = 2 needs Cin = 128 or a last 128-channel tile that is more than half full: 196 = 128 + 68 and 452 = 256 + 196 leave ragged tiles
# for both bodies, 224 / 128 are the decoder's own, 1024 fills the chip from a map smaller than one chunk
FILTER_CIN = (128, 196, 224, 228, 256, 452, 1024, 2048)


def filter_space():
    out = []
    for m in FILTER_MAPS + FILTER_MULTITAP_MAPS:
        for cout in range(52, 260 if m[1] * m[2] < 32 else 132, 4):
            for cin in (FILTER_CIN if m in FILTER_MAPS else ()):
                for k in (1, 3):
                    for wide in (False, True):
                        out.append(FShape(*m, cin, cout, k, 1 + (cout // 4) % 2 if k == 3 else 1, wide))
            for cin in (8, 12):
                out.append(FShape(*m, cin, cout, 3, 1 + (cout // 4) % 2, False))
        for cin in (8, 12):   # (multitap keeps wide column tiles only when the column blocks alone fill the chip)
            for cout in range(200, 1200, 36):
                out.append(FShape(*m, cin, cout, 3, 2, False))
    return [s for s in out if fcost(s) <= FILTER_MAX_COST]


def search_filter():
    """instance name -> [cheapest shape, cheapest 12-channel shape (multitap: 108 flattened (tap, channel) rows cut the 32-row wave blocks
    unevenly across the taps, the 72 rows of 8 channels do not), cheapest shape whose rows are no multiple of 32 and that has a channel
    tail] without repeats."""
    found = {}
    for s in filter_space():
        name = filter_instance(s)
        if name is None:
            continue
        ragged = (s.N * s.H * s.W) % 32 != 0 and s.Cin % 32 != 0 and s.Cout % 16 != 0
        for cls in ("cheap", "cin12", "ragged"):
            if (cls == "ragged" and not ragged) or (cls == "cin12" and s.Cin != 12):
                continue
            b = found.get((name, cls))
            if b is None or (fcost(s), s) < (fcost(b), b):
                found[(name, cls)] = s
    out = collections.defaultdict(list)
    for (name, _), s in sorted(found.items()):
        if s not in out[name]:
            out[name].append(s)
    return out


# ---------------------------------------------------------------------------------------------------------------- float64 references
def im2col(x, k, dil, sign=1):
    """x [N, H, W, C] -> [N H W, k k C] float64, tap-major: tap (th, tw) of pixel (h, w) reads (h + sign (th - 1) dil, w + sign (tw - 1)
    dil), zeros outside the map (stride 1, TF-SAME)."""
    import torch
    import torch.nn.functional as F
    x = x.double()
    N, H, W, C = x.shape
    if k == 1:
        return x.reshape(-1, C)
    xp = F.pad(x, (0, 0, dil, dil, dil, dil))
    cols = [xp[:, dil + sign * (th - 1) * dil: dil + sign * (th - 1) * dil + H, dil + sign * (tw - 1) * dil: dil + sign * (tw - 1) * dil + W, :]
            for th in range(k) for tw in range(k)]
    return torch.cat(cols, dim=3).reshape(N * H * W, k * k * C)


def conv_ref(x, w, dil):
    """y [N, H, W, Cout] = conv(x, w [k, k, Cin, Cout]) in float64."""
    k, _, cin, cout = w.shape
    return (im2col(x, k, dil) @ w.double().reshape(k * k * cin, cout)).reshape(*x.shape[:3], cout)


def bwd_data_ref(dy, w, dil):
    """dx [N, H, W, Cin] of the same conv: the mirrored taps of dy against w[tap][ci][co] summed over (tap, co)."""
    k, _, cin, cout = w.shape
    return (im2col(dy, k, dil, -1) @ w.double().permute(0, 1, 3, 2).reshape(k * k * cout, cin)).reshape(*dy.shape[:3], cin)


def filter_grad_ref(x, dy, k, dil):
    """dw [k, k, Cin, Cout] by float64 autograd through the im2col product."""
    import torch
    cin, cout = x.shape[3], dy.shape[3]
    w0 = torch.zeros(k * k * cin, cout, dtype=torch.float64, requires_grad=True)
    (gw,) = torch.autograd.grad(im2col(x, k, dil) @ w0, [w0], dy.double().reshape(-1, cout))
    return gw.reshape(k, k, cin, cout)
