"""The dense-conv kernel instances (csrc/conv_gemm_kernels.hpp, conv_gemm.hip) as a manifest, and a search for the cheapest shape that
makes the library's planners pick each of them.  No device work: only the planner queries are called (they answer without a GPU, with
the MI355X's 256 CUs).

Every template instantiation is separate compiled code with its own register allocation and K / column / row-group tails, so a parity
test covers an instance only if it launches it.  DECLARED lists what the launch switches can name, `search()` / `search_filter()` find
what the planners do name, UNREACHABLE says why the rest cannot be -- test_conv_instances_cpu.py holds the three together and
test_conv_instances_gpu.py launches every reached instance under parity (as memcheck.py's COVERED / EXEMPT do for the entry points).

Names are what mliis_conv2d_kernel_name prints.  Two kinds of instance have no name query of their own and get one here: the
conv1x1_stream_k<..., AIN = true> forms of mliis_conv2d_fwd_bnin ("conv1x1_stream_k<KC, NT, PREC, true>") and the filter gradients
("conv_filter_grad2_k<TMF, NT, SC, BF>", from mliis_conv2d_bwd_filter_plan; " multitap" appended for the all-taps-in-one-block path,
which is a run-time branch of the same instantiation with its own indexing)."""
import collections
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "mliis_amd", "csrc", "conv_gemm_kernels.hpp")

PREC_ID = {"fp32": 0, "bf16": 1, "fp8": 2}

# ---------------------------------------------------------------------------------------------------------------- declared instances
# MLIIS_STREAM_INSTANCES: (KC, NT, AIN form exists)
STREAM_INSTANCES = ((1, 1, 1), (1, 2, 1), (1, 3, 1), (1, 4, 1), (1, 5, 0), (1, 6, 0), (1, 7, 0), (1, 8, 0), (2, 1, 1), (2, 2, 1), (2, 3, 1),
                    (2, 4, 1), (3, 1, 1), (3, 2, 1), (4, 1, 1), (4, 2, 1), (5, 1, 1), (6, 1, 1), (7, 1, 1))
# MLIIS_KSPLIT_INSTANCES: (KC, NT)
KSPLIT_INSTANCES = ((1, 1), (1, 2), (1, 3), (1, 4), (1, 5), (1, 6), (1, 7), (2, 1), (2, 2), (2, 3), (2, 4), (3, 1), (3, 2), (4, 1),
                    (4, 2), (4, 3), (5, 1), (5, 2), (6, 1), (6, 2), (7, 1))
# launch_gemm_t: ROW(TM) over NT 1..8; TM = 1: narrow | (x_scale, split-K) in all four combinations; TM = 2: x_scale or not, never split
GEMM_TM, GEMM_NT = (1, 2), tuple(range(1, 9))
# launch_gemm_sk_t: conv_gemm_sk_k<NT, 2, false, PREC> + sk_fixup_k<NT>
SK_NT = tuple(range(1, 9))
# launch_filter_t: ROW(TMF) over NT 1..8, x_scale or not
FILTER_TMF, FILTER_NT = (1, 2), tuple(range(1, 9))

# family -> the operand precisions an instantiation exists for (launch_gemm / launch_1x1 / launch_filter and the *_bf16 / *_fp8 units)
FAMILIES = collections.OrderedDict([
    ("stream", ("fp32", "bf16", "fp8")),
    ("stream_ain", ("fp32", "bf16", "fp8")),
    ("ksplit", ("fp32", "bf16", "fp8")),
    ("gemm", ("fp32", "bf16", "fp8")),
    ("sk", ("fp32", "bf16")),          # (launch_gemm: an fp8 call never takes the stream-K pair)
    ("filter", ("fp32", "bf16")),      # (launch_filter: the backward passes of an fp8 step take the bf16 instances)
])

# family -> precision of the CALL -> how the instance rounds its two matrix-core operands before the multiply (accumulation is fp32
# everywhere): "none": fp32 operands; "bf16": round to nearest even in registers; "fp8": OCP e4m3 after the power-of-two scales
# (activations x FP8_ACT_SCALE, weights x 2^floor(log2(224 / amax)), saturating at +-448).  With an x_scale the product x * x_scale is
# formed in fp32 first and then rounded.
# The stream kernel follows the call like every other family: conv1x1_stream_k<KC, NT, PREC> reads an fp32 A, but its PREC != 0
# branches pack BOTH operands (pack_bf16x8 / pack_fp8x8 of the A rows and of the B fragments) -- the AIN forms round the finished
# batch-norm output a, not z.  (An older docstring said it kept fp32 operands in bf16 mode; launch_stream_lowp and route_conv are right.)
_CALL = {"fp32": "none", "bf16": "bf16", "fp8": "fp8"}
ROUNDING = {
    "stream": _CALL,
    "stream_ain": _CALL,
    "ksplit": _CALL,
    "gemm": _CALL,                              # (a 3x3 call in fp8 mode is a bf16 call: mliis_conv2d_fwd, and its name says so)
    "sk": {"fp32": "none", "bf16": "bf16"},
    "filter": {"fp32": "none", "bf16": "bf16"},
}


def _b(v):
    return "true" if v else "false"


def stream_name(kc, nt, prec, ain=False):
    return "conv1x1_stream_k<{}, {}, {}{}>".format(kc, nt, PREC_ID[prec], ", true" if ain else "")


def ksplit_name(kc, nt, prec):
    return "conv1x1_ksplit_k<{}, {}, 8, {}>".format(kc, nt, PREC_ID[prec])


def gemm_name(tm, nt, sc, sp, narrow, prec):
    return "conv_gemm_nk_k<{}, {}, {}, {}, {}, {}, {}>".format(tm, nt, 2 if tm == 1 else 1, _b(sc), _b(sp), _b(narrow), PREC_ID[prec])


def sk_name(nt, prec):
    return "conv_gemm_sk_k<{}, 2, false, {}>".format(nt, PREC_ID[prec])


def filter_name(tmf, nt, sc, prec, multitap):
    return "conv_filter_grad2_k<{}, {}, {}, {}>{}".format(tmf, nt, _b(sc), _b(prec == "bf16"), " multitap" if multitap else "")


def parse_name(name):
    """(kernel, [template arguments as int / bool], multitap) of an instance name."""
    m = re.fullmatch(r"(\w+)<([^>]*)>( multitap)?", name)
    args = [a.strip() == "true" if a.strip() in ("true", "false") else int(a) for a in m.group(2).split(",")]
    return m.group(1), args, m.group(3) is not None


def family_of(name):
    kernel, args, _ = parse_name(name)
    if kernel == "conv1x1_stream_k":
        return "stream_ain" if len(args) == 4 else "stream"
    return {"conv1x1_ksplit_k": "ksplit", "conv_gemm_nk_k": "gemm", "conv_gemm_sk_k": "sk", "conv_filter_grad2_k": "filter"}[kernel]


def precision_of(name):
    kernel, args, _ = parse_name(name)
    if kernel == "conv_filter_grad2_k":
        return "bf16" if args[3] else "fp32"
    p = args[2] if kernel == "conv1x1_stream_k" else args[-1]
    return {v: k for k, v in PREC_ID.items()}[p]


def declared(family, prec):
    """The instance names of a family that are compiled for one precision."""
    if prec not in FAMILIES[family]:
        return set()
    if family == "stream":
        return {stream_name(kc, nt, prec) for kc, nt, _ in STREAM_INSTANCES}
    if family == "stream_ain":
        return {stream_name(kc, nt, prec, True) for kc, nt, ain in STREAM_INSTANCES if ain}
    if family == "ksplit":
        return {ksplit_name(kc, nt, prec) for kc, nt in KSPLIT_INSTANCES}
    if family == "gemm":
        out = set()
        for nt in GEMM_NT:
            out.add(gemm_name(1, nt, False, False, True, prec))
            out |= {gemm_name(1, nt, sc, sp, False, prec) for sc in (False, True) for sp in (False, True)}
            out |= {gemm_name(2, nt, sc, False, False, prec) for sc in (False, True)}
        return out
    if family == "sk":
        return {sk_name(nt, prec) for nt in SK_NT}
    return {filter_name(tmf, nt, sc, prec, mt) for tmf in FILTER_TMF for nt in FILTER_NT for sc in (False, True) for mt in (False, True)}


def all_declared():
    return {n for fam, precs in FAMILIES.items() for p in precs for n in declared(fam, p)}


# ---------------------------------------------------------------------------------------------------------------- unreachable instances
# declared instance -> the planner line that keeps every shape away from it.  They stay compiled (removing them is a decision about
# the build, not about the tests); a planner change that reaches one makes test_conv_instances_cpu.py fail until its entry goes.
def _unreachable():
    u = {}
    for prec in ("fp32", "bf16", "fp8"):
        for kc, nt, ain in STREAM_INSTANCES:
            if nt >= 3:
                why = "stream_plan: `if (nt > 2) nt = 2` caps the column tiles per wave at two"
                u[stream_name(kc, nt, prec)] = why
                if ain:
                    u[stream_name(kc, nt, prec, True)] = why
        for nt in GEMM_NT:
            if nt >= 5:
                for sc in (False, True):
                    u[gemm_name(1, nt, sc, True, False, prec)] = (
                        "plan_gemm: K is split only while blocks * 2 <= num_cus; such a grid has gx < num_cus and gx * gy < kGemmFill * num_cus, "
                        "so the narrowing loop `g.nt = (g.nt + 1) / 2` has already cut nt to min_nt = 4 or below")
            elif nt >= 3:
                u[gemm_name(1, nt, True, True, False, prec)] = (
                    "mliis_conv2d_fwd takes an x_scale for 1x1 convs only, and plan_gemm narrows a 1x1 grid small enough to split K down to "
                    "min_nt = 2 (`const int min_nt = ntaps == 9 ? 4 : 2`)")
        for nt in GEMM_NT:
            if prec == "fp8":
                u[gemm_name(1, nt, False, False, True, prec)] = (
                    "mliis_conv2d_fwd: `if (precision == MLIIS_PREC_FP8 && ksize != 1) precision = MLIIS_PREC_BF16` -- the narrow form is a "
                    "3x3 conv, which never launches with fp8 operands")
                if 3 <= nt <= 4:
                    u[gemm_name(1, nt, False, True, False, prec)] = (
                        "fp8 operands are for 1x1 convs (mliis_conv2d_fwd turns a 3x3 call into bf16), and plan_gemm narrows a 1x1 grid small "
                        "enough to split K down to min_nt = 2")
    # (stream-K and the filter gradients: every declared instance is reached -- the multitap path with eight column tiles only by a 3x3
    #  conv from 8 | 12 channels to some 370 and more, where three column blocks x 96 slabs are the 256 blocks plan_filter wants)
    return u


UNREACHABLE = _unreachable()


def reachable_1x1(family):
    """The (KC, NT) pairs of a 1x1 family that some shape reaches: the header's list without the UNREACHABLE ones."""
    if family == "stream":
        return [(kc, nt) for kc, nt, _ in STREAM_INSTANCES if stream_name(kc, nt, "fp32") not in UNREACHABLE]
    return [(kc, nt) for kc, nt in KSPLIT_INSTANCES if ksplit_name(kc, nt, "fp32") not in UNREACHABLE]


def parse_header_lists(path=HEADER):
    """(stream, ksplit) instance tuples as the X(...) entries of the two header macros spell them."""
    src = open(path).read()

    def macro(name):
        m = re.search(r"#define\s+" + name + r"\(X\)((?:[^\n]*\\\n)*[^\n]*)\n", src)
        assert m, name
        return tuple(tuple(int(v) for v in e.split(",")) for e in re.findall(r"X\(([^)]*)\)", m.group(1)))

    return macro("MLIIS_STREAM_INSTANCES"), macro("MLIIS_KSPLIT_INSTANCES")


# ---------------------------------------------------------------------------------------------------------------- shape search
# A shape is what a plain call has: dense leading dimensions, no accumulate, no border bias, a workspace given.
Shape = collections.namedtuple("Shape", "N H W K Nout ksize scale")


def rows(s):
    return s.N * s.H * s.W


def cost(s):
    return rows(s) * s.K * s.ksize * s.ksize * s.Nout


def missing_tails(s, kmod):
    """How many of the three tails a shape lacks: rows, K (per tap) and Nout that are NOT multiples of 16 / kmod / 16."""
    return int(rows(s) % 16 == 0) + int(s.K % kmod == 0) + int(s.Nout % 16 == 0)


MAX_COST = 3 * 10 ** 9   # multiply-adds of the largest shape a search may keep (the float64 reference runs on the host)
NUM_CUS = 256            # the MI355X's; only the `steady` rule of the two 1x1 kernels below uses it

# maps: tiny ones (fewer than 16 rows, fewer than 16 pixels per image), both sides of the 1024-row stream threshold, of ksplit's 8192-
# and 32768-row rules, of the 256 x 64 rows that fill the chip once and of the 4 x 256 x 64 rows behind which the GEMM takes 128-row
# tiles; (2, 63, 65) / (2, 91, 93) / (2, 257, 257): maps on which every workgroup of a 1x1 kernel gets a second row group
MAPS = ((1, 3, 5), (5, 3, 3), (2, 3, 5), (1, 7, 9), (2, 5, 7), (3, 9, 11), (2, 13, 15), (2, 23, 23), (1, 47, 47), (1, 73, 75), (2, 63, 65),
        (3, 53, 53), (1, 105, 107), (1, 127, 129), (1, 128, 129), (1, 129, 131), (2, 91, 93), (1, 181, 183), (1, 257, 257), (2, 257, 257))
_COLS = tuple(16 * t - d for t in range(1, 9) for d in (4, 8)) + (136, 140, 152, 200, 236)   # column tails of 12 and 8, every pick_nt width


def conv_space():
    """The plain forward calls the search asks about, family by family (the planners' own thresholds)."""
    out = []
    # stream: K = 16 KC - 4 | 16 KC - 12, at least 1024 rows, one to a few column tiles
    for kc in range(1, 8):
        for K in (16 * kc - 4, 16 * kc - 12):
            for nout in (8, 12, 24, 28, 40, 44, 56, 72, 88):
                for m in ((2, 23, 23), (2, 257, 257)):
                    out.append(Shape(*m, K, nout, 1, False))
    # ksplit: K = 128 KC - 4 j, 16 .. 32768 rows on both sides of the 8192-row rule, gated or not (gated maps below 16 pixels: GEMM)
    for kc in range(1, 8):
        for K in (128 * kc - 4, 128 * kc - 12):
            for m in ((2, 5, 7), (2, 3, 5), (2, 13, 15), (2, 63, 65), (3, 53, 53), (2, 91, 93)):
                for nout in [c for c in range(8, 244, 4) if c % 16 in (8, 12)]:
                    for sc in (False, True):
                        out.append(Shape(*m, K, nout, 1, sc))
    # GEMM (both tile heights, split or not, narrow, stream-K): 1x1 with and without the gate, 3x3
    for m in MAPS:
        for nout in _COLS:
            for K in (4, 12, 20, 28, 36, 72, 100, 116, 136, 200, 264, 520, 900, 1000):
                for sc in (False, True):
                    out.append(Shape(*m, K, nout, 1, sc))
            for K in (4, 12, 20, 28, 36, 40, 60, 72, 136):
                out.append(Shape(*m, K, nout, 3, False))
    return [s for s in out if cost(s) <= MAX_COST]


def filter_space():
    out = []
    for m in MAPS:
        if m[1] * m[2] < 9:
            continue
        for nout in _COLS:
            for C in (4, 8, 12, 24, 64, 72, 128, 136, 200):
                for k in (1, 3):
                    out.append(Shape(*m, C, nout, k, False))
        for C in (8, 12):   # (multitap with eight column tiles: three column blocks)
            out.append(Shape(*m, C, 372, 3, False))
    return [s for s in out if cost(s) <= MAX_COST]


# Two shapes per instance.  "tails": the cheapest shape with all three tails -- usually one pass of every loop, the prologue feeding the
# epilogue.  "steady": the cheapest one in which the kernel's main loop comes round again with its prefetch in flight -- every workgroup
# of the 1x1 kernels streams a second row group (their grids are sized by the CU count, not by the rows), the LDS-tiled GEMM runs at
# least four K chunks per block (its pipeline is two chunks deep), a filter-gradient block at least five 32-pixel chunks (its loop is
# unrolled by four).  One shape may be both.
CLASSES = ("tails", "steady")


def _ok_for(fam, s, args):
    """Shapes the search refuses for a family although they launch it: a ksplit K must end inside the LAST wave's last 16-wide K
    group (K = 520 is KC = 5 too, but leaves the eighth wave's slice empty and the seventh's full: no K tail at all)."""
    if fam == "ksplit":
        return 128 * args[0] - 16 < s.K < 128 * args[0]
    return True


def _steady(fam, s, args, plan=None):
    rg = -(-rows(s) // 16)
    if fam == "stream":        # stream_plan: about 16 waves per CU, a row group per wave and round
        return rg >= 2 * 16 * NUM_CUS
    if fam == "ksplit":        # ksplit_plan: one workgroup per CU up to 8192 rows and for KC = 7, two beyond
        return rg >= 2 * NUM_CUS * (1 if (rows(s) <= 8192 or args[0] >= 7) else 2)
    if fam in ("gemm", "sk"):  # plan = (tm, nt, splits) of mliis_conv2d_plan
        return -(-(-(-s.ksize * s.ksize * s.K // 32)) // plan[2]) >= 4
    return min(rows(s), plan[6]) >= 5 * 32   # filter: plan = mliis_conv2d_bwd_filter_plan, [6] = rows per slab


def _keep(found, name, s, kmod, steady):
    for cls in CLASSES:
        if cls == "steady" and not steady:
            continue
        b = found.get((name, cls))
        if b is None or (missing_tails(s, kmod), cost(s), s) < (missing_tails(b, kmod), cost(b), b):
            found[(name, cls)] = s


def search(prec):
    """(instance name, class) -> the cheapest plain shape (all three tails preferred) whose forward call with this precision launches
    it; the stream_ain names ride on the stream shapes that mliis_conv2d_fwd_bnin accepts."""
    from mliis_amd import ops
    found = {}
    for s in conv_space():
        if prec == "fp8" and s.ksize != 1:
            continue   # (such a call is a bf16 call)
        name = ops.conv2d_kernel_name(s.N, s.H, s.W, s.K, s.Nout, s.ksize, s.scale, prec)
        fam, args = family_of(name), parse_name(name)[1]
        if not _ok_for(fam, s, args):
            continue
        plan = ops.conv2d_plan(s.N, s.H, s.W, s.K, s.Nout, s.ksize) if fam in ("gemm", "sk") else None
        _keep(found, name, s, 16 if fam in ("stream", "ksplit") else 32, _steady(fam, s, args, plan))
    for (name, cls), s in list(found.items()):
        if family_of(name) == "stream" and ops.conv2d_fwd_bnin_ok(s.N, s.H, s.W, s.K, s.Nout):
            found[(name[:-1] + ", true>", cls)] = s
    return found


def filter_plan(s):
    import ctypes as C
    from mliis_amd._lib import lib
    plan = (C.c_int * 7)()
    lib.call("mliis_conv2d_bwd_filter_plan", s.N, s.H, s.W, s.K, s.Nout, s.ksize, C.cast(plan, C.c_void_p))
    return tuple(plan)   # (TMF, NT, multitap, gx, gy, gz, rows_per_split)


def search_filter(prec):
    """(filter-gradient instance name, class) -> shape, with and without the x_scale operand (the plan does not depend on it)."""
    found = {}
    for s in filter_space():
        plan = filter_plan(s)
        for sc in (False, True):
            _keep(found, filter_name(plan[0], plan[1], sc, prec, plan[2]), s._replace(scale=sc), 16, _steady("filter", s, None, plan))
    return found


def reached():
    """Every instance name some searched shape launches -> (its one or two shapes, precision of the call)."""
    out = {}
    for prec in ("fp32", "bf16", "fp8"):
        both = dict(search(prec))
        if prec != "fp8":
            both.update(search_filter(prec))
        for (name, cls), s in sorted(both.items()):
            shapes = out.setdefault(name, ([], prec))[0]
            if s not in shapes:
                shapes.append(s)
    return out


def cases(family, prec, table):
    """[(name, shape)] of one family and precision out of reached(), in a fixed order."""
    return sorted((n, s) for n, (shapes, p) in table.items() if family_of(n) == family and p == prec for s in shapes)
