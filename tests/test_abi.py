"""The C-ABI library loads, exports every symbol include/mliis_hip.h declares, and the ctypes table matches the header
(argument count and scalar kinds).  No compute calls: runs without a GPU."""
import ctypes as C
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "mliis_hip.h")


def _decls():
    src = open(HEADER).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    out = {}
    for m in re.finditer(r"([\w\s\*]+?)\b(mliis_\w+)\s*\(([^;{]*?)\)\s*;", src):
        ret, name, args = m.group(1).strip(), m.group(2), m.group(3).strip()
        params = [] if args in ("", "void") else [a.strip() for a in args.split(",")]
        out[name] = (ret, params)
    return out


def _kind(param: str):
    if "*" in param or "hipStream_t" in param:
        return C.c_void_p
    if param.startswith("long long"):
        return C.c_longlong
    if param.startswith("size_t"):
        return C.c_size_t
    if param.startswith("float"):
        return C.c_float
    if param.startswith("int"):
        return C.c_int
    raise AssertionError("unknown param kind: " + param)


def test_header_matches_ctypes_table():
    from mliis_amd._lib import SIGNATURES
    decls = _decls()
    assert set(decls) == set(SIGNATURES), set(decls) ^ set(SIGNATURES)
    for name, (ret, params) in decls.items():
        res, argtypes = SIGNATURES[name]
        assert len(params) == len(argtypes), name
        for p, a in zip(params, argtypes):
            k = _kind(p)
            if k is C.c_void_p:
                assert a is C.c_void_p or issubclass(a, C._Pointer), (name, p)
            else:
                assert a is k, (name, p, a)


def test_library_exports_every_symbol():
    from mliis_amd._lib import LIB_PATH, lib
    if not os.path.exists(LIB_PATH):
        import __graft_entry__ as g
        g.build()
    dll = lib.load()
    for name in _decls():
        assert hasattr(dll, name), name
    assert lib.size("mliis_version") >= 100


def test_workspace_queries_need_no_gpu():
    from mliis_amd._lib import lib
    assert lib.size("mliis_colreduce_workspace_floats", 100352, 32, 1, 2) > 0
    assert lib.size("mliis_dwconv_bwd_filter_workspace_floats", 8, 112, 112, 32, 3, 1) > 0
    assert lib.size("mliis_conv2d_bwd_filter_workspace_floats", 8, 56, 56, 360, 112, 3) >= 9 * 360 * 112
    assert lib.size("mliis_softmax_ce_workspace_floats", 8, 224, 224) > 0
    assert lib.size("mliis_colreduce_workspace_floats", 10, 30, 1, 1) == 0  # C % 4 != 0 -> rejected


# The 1x1 instances the planners may pick: the lists of test_the_1x1_kernel_instances_fit_the_residency_their_planner_assumes
# (test_ops_gpu.py), and the three KC * NT = 12 ksplit instances of the small maps, which that test leaves out because they run one
# workgroup per CU by design (conv_gemm_kernels.hpp: MLIIS_KSPLIT_INSTANCES).
STREAM_INSTANCES = {(1, 1), (1, 2), (1, 3), (1, 4), (2, 1), (2, 2), (2, 3), (3, 1), (3, 2), (4, 1), (4, 2), (5, 1), (6, 1), (7, 1)}
KSPLIT_INSTANCES = {(1, n) for n in range(1, 8)} | {(2, 1), (2, 2), (2, 3), (2, 4), (3, 1), (3, 2), (4, 1), (4, 2), (5, 1), (6, 1), (7, 1)} | {
    (4, 3), (5, 2), (6, 2)}


def test_the_dense_conv_planner_queries_agree_with_each_other():
    """The kernel-name query and conv2d_fwd_bnin_ok are two views of one routing decision (route_conv in csrc/conv_gemm.hip): plan.py
    lays out the group-blocked tensors by the first and fuses the project batch norm by the second.  For a plain fp32 1x1 shape the
    streamed name and bnin_ok must coincide -- including N = 64, 112x112, Cout = 672, whose output passes 2 GiB, where the name query
    once kept saying conv1x1_stream_k although the launch takes the GEMM.  No compute calls."""
    import itertools
    from mliis_amd import ops
    seen = {"conv1x1_stream_k": set(), "conv1x1_ksplit_k": set()}
    big = 0
    for N, HW, cred, nout in itertools.product((1, 2, 8, 64), (4, 7, 14, 28, 56, 112), (8, 16, 24, 40, 96, 112, 116, 144, 240, 480, 672, 1152),
                                               (8, 16, 24, 40, 80, 112, 136, 240, 672)):
        plain = ops.conv2d_kernel_name(N, HW, HW, cred, nout, 1)
        assert ops.conv2d_fwd_bnin_ok(N, HW, HW, cred, nout) == plain.startswith("conv1x1_stream_k"), (N, HW, cred, nout, plain)
        if N * HW * HW * max(cred, nout) * 4 >= 2 ** 31:
            big += 1
            assert plain.startswith("conv_gemm_"), (N, HW, cred, nout, plain)   # (the 1x1 kernels use 32-bit byte offsets)
        for prec in ("fp32", "bf16", "fp8"):
            assert ops.conv2d_kernel_name(N, HW, HW, cred, nout, 3, False, prec).startswith("conv_gemm_"), (N, HW, cred, nout, prec)
            for has_scale in (False, True):
                m = re.match(r"(conv1x1_\w+_k)<(\d+), (\d+), ", ops.conv2d_kernel_name(N, HW, HW, cred, nout, 1, has_scale, prec))
                if m:
                    seen[m.group(1)].add((int(m.group(2)), int(m.group(3))))
    assert big > 0 and seen["conv1x1_stream_k"] and seen["conv1x1_ksplit_k"]   # (the grid reaches every rule it is meant to)
    assert seen["conv1x1_stream_k"] <= STREAM_INSTANCES, seen["conv1x1_stream_k"] - STREAM_INSTANCES
    assert seen["conv1x1_ksplit_k"] <= KSPLIT_INSTANCES, seen["conv1x1_ksplit_k"] - KSPLIT_INSTANCES


def test_missing_library_fails_loudly(monkeypatch, tmp_path):
    import mliis_amd._lib as L
    fresh = L._Lib()
    monkeypatch.setattr(L, "LIB_PATH", str(tmp_path / "nope.so"))
    with pytest.raises(L.MliisError):
        fresh.load()
