"""The dense-conv instance manifest (tests/conv_instances.py) against the header it describes and against the library's planners:
the lists agree with the header macros, and every declared instance is either reached by a searched shape or has an UNREACHABLE entry
that names the planner line in its way.  The planner queries answer without a GPU (num_cus() falls back to the MI355X's 256 CUs)."""
import os

import pytest

import conv_instances as CI


@pytest.fixture(scope="module")
def table():
    from mliis_amd._lib import LIB_PATH
    if not os.path.exists(LIB_PATH):
        import __graft_entry__ as g
        g.build()
    return CI.reached()


def test_manifest_lists_equal_the_header_macros():
    stream, ksplit = CI.parse_header_lists()
    assert stream == CI.STREAM_INSTANCES, set(stream) ^ set(CI.STREAM_INSTANCES)
    assert ksplit == CI.KSPLIT_INSTANCES, set(ksplit) ^ set(CI.KSPLIT_INSTANCES)
    assert len(stream) == 19 and len(ksplit) == 21
    # what the header's comments promise of them
    assert all(kc * nt <= 8 and 1 <= kc <= 7 for kc, nt, _ in stream)
    assert all((kc * nt <= 8 or (kc >= 4 and kc * nt <= 12)) and nt <= 7 and 1 <= kc <= 7 for kc, nt in ksplit)


def test_the_header_parser_sees_an_added_pair(tmp_path):
    """A pair added to either macro without a manifest entry must fail the comparison above: the parser reads what is there."""
    src = open(CI.HEADER).read()
    edited = src.replace("X(7, 1)\n", "X(7, 1) X(8, 1)\n", 1).replace("X(6, 1, 1) X(7, 1, 1)\n", "X(6, 1, 1) X(7, 1, 1) X(3, 3, 0)\n", 1)
    assert edited.count("X(8, 1)") == 1 and edited.count("X(3, 3, 0)") == 1
    p = tmp_path / "conv_gemm_kernels.hpp"
    p.write_text(edited)
    stream, ksplit = CI.parse_header_lists(str(p))
    assert stream == CI.STREAM_INSTANCES + ((3, 3, 0),) and ksplit == CI.KSPLIT_INSTANCES + ((8, 1),)


def test_names_parse_back_to_their_family_and_precision():
    for fam, precs in CI.FAMILIES.items():
        assert set(CI.ROUNDING[fam]) == set(precs)
        for p in precs:
            names = CI.declared(fam, p)
            assert names and all(CI.family_of(n) == fam and CI.precision_of(n) == p for n in names), (fam, p)
    assert len(CI.all_declared()) == 3 * 19 + 3 * 15 + 3 * 21 + 3 * 56 + 2 * 8 + 2 * 64
    assert set(CI.UNREACHABLE) <= CI.all_declared()
    assert all(("plan" in why or "mliis_conv2d_fwd" in why) and len(why) > 40 for why in CI.UNREACHABLE.values())


def test_every_declared_instance_is_reached_or_has_a_reason(table):
    declared, hit, never = CI.all_declared(), set(table), set(CI.UNREACHABLE)
    assert hit <= declared, sorted(hit - declared)               # the planners name nothing the launch switches do not have
    assert not (hit & never), sorted(hit & never)                # a stale UNREACHABLE entry
    assert hit | never == declared, sorted(declared - hit - never)   # an instance no parity test can launch, and nobody said why
    # the stream kernel's cap: eight of its 19 instances, in every precision and in the batch-norm-on-load form
    assert sorted(CI.reachable_1x1("stream")) == sorted((kc, nt) for kc, nt, _ in CI.STREAM_INSTANCES if nt <= 2)
    assert CI.reachable_1x1("ksplit") == list(CI.KSPLIT_INSTANCES)


def test_searched_shapes_have_their_tails_and_stay_small(table):
    for name, s in ((n, s) for n, (shapes, _) in table.items() for s in shapes):
        fam = CI.family_of(name)
        assert CI.cost(s) <= CI.MAX_COST, (name, s)
        assert CI.missing_tails(s, 16 if fam in ("stream", "stream_ain", "ksplit", "filter") else 32) == 0, (name, s)
        assert (s.K % 4, s.Nout % 4) == (0, 0)
        if fam == "gemm":   # the name's fields are the plan's
            from mliis_amd import ops
            _, (tm, nt, _, sc, sp, narrow, _), _ = CI.parse_name(name)
            ptm, pnt, psplits = ops.conv2d_plan(s.N, s.H, s.W, s.K, s.Nout, s.ksize)
            assert (tm, nt, sp) == (ptm, pnt, psplits > 1) and sc == s.scale and narrow == (s.ksize == 3 and s.K < 32), (name, s)


def test_the_1x1_instances_get_a_k_tail_in_the_last_wave_and_a_second_row_group(table):
    """What the cheapest shape alone would miss: K = 520 launches conv1x1_ksplit_k<5, ...> as well but leaves the eighth wave without a
    single channel, and on a map of 30 rows no workgroup of either 1x1 kernel comes round its row-group loop a second time."""
    for name, (shapes, _) in table.items():
        fam, (kc, nt) = CI.family_of(name), CI.parse_name(name)[1][:2]
        if fam == "ksplit":
            assert all(128 * kc - 16 < s.K < 128 * kc for s in shapes), (name, shapes)
            assert any(-(-CI.rows(s) // 16) >= 2 * CI.NUM_CUS for s in shapes) and any(CI.rows(s) < 1024 for s in shapes), (name, shapes)
        if fam in ("stream", "stream_ain"):
            assert all(16 * kc - 16 < s.K < 16 * kc for s in shapes), (name, shapes)
            assert any(-(-CI.rows(s) // 16) >= 32 * CI.NUM_CUS for s in shapes) and any(CI.rows(s) < 2048 for s in shapes), (name, shapes)
        if fam in ("gemm", "sk") and len(shapes) == 2:
            assert shapes[0] != shapes[1]


def test_routing_facts_the_search_spaces_rely_on():
    from mliis_amd import ops
    # a gated 1x1 conv on maps of fewer than 16 pixels, and any 1x1 conv of fewer than 16 rows, fall to the GEMM; so does a gated short-K one
    assert ops.conv2d_kernel_name(5, 3, 3, 244, 40, 1, True).startswith("conv_gemm_nk_k")
    assert ops.conv2d_kernel_name(5, 3, 3, 244, 40, 1, False).startswith("conv1x1_ksplit_k")
    assert ops.conv2d_kernel_name(1, 3, 5, 244, 40, 1, False).startswith("conv_gemm_nk_k")
    assert ops.conv2d_kernel_name(2, 23, 23, 44, 40, 1, True).startswith("conv_gemm_nk_k<1, 2, 2, true, false, false")
    assert ops.conv2d_kernel_name(2, 23, 23, 44, 40, 1, False) == "conv1x1_stream_k<3, 2, 0>"
    # both sides of ksplit's 8192-row rule: twelve B-fragment quads on the small maps only
    assert ops.conv2d_kernel_name(2, 5, 7, 508, 44, 1) == "conv1x1_ksplit_k<4, 3, 8, 0>"
    assert ops.conv2d_kernel_name(3, 53, 53, 508, 44, 1) == "conv1x1_ksplit_k<4, 2, 8, 0>"
    # a long-K 1x1 conv beyond ksplit's rows whose tile count leaves a remainder: the stream-K pair in fp32 / bf16; an fp8 call has no
    # such form and launches the plan's tiles whole (launch_gemm) -- the name query says what runs
    assert ops.conv2d_kernel_name(9, 64, 64, 512, 112, 1) == "conv_gemm_sk_k<7, 2, false, 0>"
    assert ops.conv2d_kernel_name(9, 64, 64, 512, 112, 1, False, "bf16") == "conv_gemm_sk_k<7, 2, false, 1>"
    assert ops.conv2d_kernel_name(9, 64, 64, 512, 112, 1, False, "fp8") == "conv_gemm_nk_k<1, 7, 2, false, false, false, 2>"
    assert ops.conv2d_kernel_name(8, 56, 56, 72, 112, 3, False, "fp8") == "conv_gemm_sk_k<7, 2, false, 1>"   # (a 3x3 call in fp8 mode is a bf16 call)
