"""The marching-depthwise instance table and geometry mirror (tests/dwmarch_instances.py) against the source they describe and the
library's block-count queries, which are host code and answer without a GPU: the table is the cross product the launch switches of
csrc/dwmarch.hip can name, the mirror's workgroup count is the library's for every case, and every case has the march it is there
for -- bands, chunks and tails in the edge shapes, one chunk of an odd number of steps with a partial last one in the long shapes."""
import itertools
import os
import re

import pytest

import dwmarch_instances as DI

pytestmark = pytest.mark.skipif(DI.target_overridden(), reason=DI.ENV_TARGET + " is set: the chunk counts are not the default ones the mirror describes")

SOURCE = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "mliis_amd", "csrc", "dwmarch.hip")


@pytest.fixture(scope="module")
def queries():
    from mliis_amd._lib import LIB_PATH
    if not os.path.exists(LIB_PATH):
        import __graft_entry__ as g
        g.build()
    from mliis_amd import ops
    return ops.lib.raw("mliis_dwconv_bn_fwd_blocks"), ops.lib.raw("mliis_dwconv_bn_bwd_blocks")


def test_the_table_is_the_cross_product_of_the_launch_switches():
    inst = DI.INSTANCES
    assert len(inst) == len(set(inst)) == 60
    by = {e: [i for i in inst if i.entry == e] for e in ("fwd", "bwd", "fused")}
    assert (len(by["fwd"]), len(by["bwd"]), len(by["fused"])) == (24, 24, 12)
    assert sum(i.s == 1 for i in by["bwd"]) == sum(i.s == 2 for i in by["bwd"]) == 12
    assert len({DI.kernel_name(i) for i in inst}) == 60
    # dwm_types_ok restated: of the four (ta, tb) combinations each direction admits three
    types = ("f32", "bf16")
    assert {p for p in itertools.product(types, types) if DI.types_ok(False, *p)} == set(DI.FWD_PAIRS)
    assert {p for p in itertools.product(types, types) if DI.types_ok(True, *p)} == set(DI.BWD_PAIRS)
    want = {DI.Instance("fwd", k, s, bn, ta, tb) for k in (3, 5) for s in (1, 2) for bn in (True, False) for ta in types for tb in types
            if DI.types_ok(False, ta, tb)}
    want |= {DI.Instance("bwd", k, s, bn, ta, tb) for k in (3, 5) for s in (1, 2) for bn in (True, False) for ta in types for tb in types
             if DI.types_ok(True, ta, tb)}
    want |= {DI.Instance("fused", k, s, True, ta, tb) for k in (3, 5) for s in (1, 2) for ta in types for tb in types if DI.types_ok(True, ta, tb)}
    assert set(inst) == want
    assert all(i.bn for i in by["fused"])          # (DYBN: always with the batch norm in front)


def test_the_source_still_has_the_switches_the_table_describes():
    """Nine launch lines name the kernels by template parameter; a tenth, or a new storage-type rule, needs a table entry."""
    src = open(SOURCE).read()
    launches = re.findall(r"hipLaunchKernelGGL\(\((dwm_\w+)<([^>]*)>\)", src)
    assert sorted(launches) == sorted([
        ("dwm_conv_k", "K, S, PRE, BWD, false, float, float"), ("dwm_conv_k", "K, S, PRE, BWD, false, bf16s, bf16s"),
        ("dwm_conv_k", "K, S, PRE, BWD, false, bf16s, float"), ("dwm_conv_k", "K, S, PRE, BWD, false, float, bf16s"),
        ("dwm_bwd_s2_k", "K, PRE, false, float, float"), ("dwm_bwd_s2_k", "K, PRE, false, bf16s, bf16s"), ("dwm_bwd_s2_k", "K, PRE, false, bf16s, float"),
        ("dwm_conv_k", "K, 1, true, true, true, TA, TB"), ("dwm_bwd_s2_k", "K, true, true, TA, TB")]), launches
    assert "return g_dwm_target ? g_dwm_target : (bwd ? 256 : 448);" in src
    assert (DI.TARGET_FWD, DI.TARGET_BWD) == (448, 256)


def test_every_declared_instance_is_reached_or_has_a_reason():
    reached = {c.inst for c in DI.cases()}
    assert not (reached & set(DI.UNREACHABLE))
    assert reached | set(DI.UNREACHABLE) == set(DI.INSTANCES)
    assert all(len(why) > 40 for why in DI.UNREACHABLE.values())
    for i in reached:
        kinds = {c.kind for c in DI.cases() if c.inst == i}
        assert kinds == {"edge", "long"}, (i, kinds)
    ids = [DI.case_id(c) for c in DI.cases()]
    assert len(ids) == len(set(ids))


def test_the_mirror_counts_the_librarys_workgroups(queries):
    fwd_blocks, bwd_blocks = queries
    shapes = {c.shape for c in DI.cases()} | {(2, 14, 14, 32), (1, 33, 61, 36), (8, 112, 112, 32), (64, 112, 112, 32), (2, 41, 63, 44), (1, 1, 9, 8)}
    for (N, H, W, C), k, s in itertools.product(sorted(shapes), DI.KS, DI.STRIDES):
        assert DI.geom_fwd(N, H, W, C, k, s).blocks == fwd_blocks(N, H, W, C, k, s), ("fwd", N, H, W, C, k, s)
        assert DI.geom_bwd(N, H, W, C, k, s).blocks == bwd_blocks(N, H, W, C, k, s), ("bwd", N, H, W, C, k, s)
    for c in DI.cases():
        N, H, W, C = c.shape
        q = fwd_blocks if c.inst.entry == "fwd" else bwd_blocks
        assert DI.geom(c.inst, c.shape).blocks == q(N, H, W, C, c.inst.k, c.inst.s) > 0, DI.case_id(c)
    # the single chunk of a real run: N = 64, the size the launch targets were tuned at
    g = DI.geom_fwd(64, 112, 112, 32, 3, 1)
    assert (g.chunks, g.steps) == (1, 28) and DI.geom_bwd(64, 112, 112, 32, 3, 1).steps == 28


def test_edge_cases_have_bands_chunks_and_tails():
    for c in DI.cases():
        if c.kind != "edge":
            continue
        g, C = DI.geom(c.inst, c.shape), c.shape[3]
        assert g.bands >= 2 and C % 32 != 0 and -(-C // 32) == 2, DI.case_id(c)
        assert g.chunks >= 2 and g.steps == 2, (DI.case_id(c), g)
        assert c.shape[0] == 9                                   # image groups 8 + 1 in dwm_dybn_setup
        # a narrower last band -- but for the stride-2 backward at W = 35 (18 patch columns = 9 + 9), whose companion shape has it
        if c.inst.entry != "fwd" and c.inst.s == 2 and c.shape == DI.SHAPES[2]["edge"]:
            assert (g.bw, g.last_bw) == (9, 9)
        else:
            assert g.last_bw < g.bw, (DI.case_id(c), g)
    for i in DI.INSTANCES:
        assert any(DI.geom(i, c.shape).last_bw < DI.geom(i, c.shape).bw for c in DI.cases() if c.inst == i and c.kind == "edge"), i
    # the stride-2 forward's last chunk is a single step
    assert {DI.geom(c.inst, c.shape).last_steps for c in DI.cases() if c.kind == "edge" and c.inst.entry == "fwd" and c.inst.s == 2} == {1}


def test_long_cases_march_one_chunk_of_an_odd_number_of_steps():
    reached = {}
    for c in DI.cases():
        if c.kind != "long":
            continue
        g, (N, _, _, C) = DI.geom(c.inst, c.shape), c.shape
        direction = "fwd" if c.inst.entry == "fwd" else "bwd"
        assert N * -(-C // 32) * g.bands == 240 and g.chunks == 1, (DI.case_id(c), g)
        assert g.steps == g.last_steps and g.steps % 2 == 1 and g.steps >= DI.MIN_STEPS[direction, c.inst.s], (DI.case_id(c), g)
        assert g.bands == 2 and g.last_bw < g.bw and C % 32 == 28 and N == 15
        # a partial last step -- but for the stride-2 backward at H = 35 (18 patch rows = 9 whole steps), whose companion shape has it
        if direction == "bwd" and c.inst.s == 2 and c.shape == DI.SHAPES[2]["long"]:
            assert (g.rows, g.unit) == (18, 2)
        else:
            assert g.rows % g.unit != 0, (DI.case_id(c), g)
        reached.setdefault((direction, c.inst.s), set()).add(g.steps)
    assert reached == {("fwd", 1): {7}, ("fwd", 2): {5}, ("bwd", 1): {7}, ("bwd", 2): {9}}
    for i in DI.INSTANCES:
        assert any(DI.geom(i, c.shape).rows % DI.geom(i, c.shape).unit for c in DI.cases() if c.inst == i and c.kind == "long"), i


def test_the_older_shape_lists_stay_short_of_the_loops_loads():
    """What the long cases are for: over the shapes of test_dwmarch_gpu.py and the depthwise cases of test_bf16_storage_gpu.py no
    stride-1 forward chunk marches more than three steps, and test_dwmarch_shapes never more than two in either direction."""
    shapes15 = [(3, 1, 14, 14, 32, 2), (3, 2, 16, 16, 24, 2), (5, 1, 14, 14, 40, 2), (5, 2, 28, 28, 16, 2), (3, 2, 15, 17, 8, 2), (5, 2, 9, 11, 8, 3),
                (3, 1, 5, 3, 4, 2), (5, 1, 7, 30, 144, 1), (3, 1, 33, 61, 36, 1), (5, 1, 37, 35, 12, 2), (3, 2, 37, 65, 20, 1), (5, 2, 41, 63, 44, 1),
                (3, 1, 1, 1, 4, 1), (5, 2, 2, 2, 4, 2), (3, 2, 1, 9, 8, 1)]
    for k, s, H, W, C, N in shapes15:
        assert DI.geom_fwd(N, H, W, C, k, s).steps <= 2 and DI.geom_bwd(N, H, W, C, k, s).steps <= 2
    baseline = [(k, s, H, H, C, 8 if H <= 112 else 2) for k, s, H, C in
                [(3, 1, 112, 32), (3, 2, 112, 96), (3, 1, 56, 144), (5, 2, 56, 144), (5, 1, 28, 240), (3, 2, 28, 240), (3, 1, 14, 480), (5, 1, 14, 672),
                 (5, 2, 96, 144), (3, 1, 48, 192)]]
    fused = [(3, 1, 28, 28, 40, 3), (3, 2, 30, 34, 24, 2), (5, 2, 28, 28, 16, 2), (5, 1, 14, 20, 8, 2), (3, 1, 56, 56, 144, 8), (3, 2, 112, 112, 96, 8),
             (5, 2, 56, 56, 144, 8), (3, 1, 9, 7, 4, 1)]
    bf16 = [(3, 1, 28, 28, 48, 3), (3, 2, 28, 28, 48, 3), (5, 1, 28, 28, 40, 3), (5, 2, 28, 28, 40, 3), (3, 1, 30, 30, 32, 3), (5, 2, 17, 17, 8, 3),
            (3, 1, 28, 28, 32, 3), (3, 1, 14, 14, 24, 3)]
    s1 = [DI.geom_fwd(N, H, W, C, k, s).steps for k, s, H, W, C, N in shapes15 + baseline + bf16 if s == 1]
    assert max(s1) == 3
    assert max(DI.geom_fwd(N, H, W, C, k, s).steps for k, s, H, W, C, N in shapes15 + baseline + bf16 if (k, s) == (5, 1)) <= 2
    assert all(DI.geom_fwd(N, H, W, C, k, s).steps <= 2 and DI.geom_bwd(N, H, W, C, k, s).steps <= 2 for k, s, H, W, C, N in bf16)
    assert max(DI.geom_bwd(N, H, W, C, k, s).steps for k, s, H, W, C, N in fused if (k, s) == (5, 1)) <= 2
