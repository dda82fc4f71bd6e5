"""The Tversky region term, the host half: the flag and the Learner argument it becomes, libmliis_region.so's build and exported ABI against
include/mliis_region.h, its host-only queries and refusals, and the reference of tests/tversky_ref.py against the oracle's loss
(alpha = beta = 1) and against the closed-form gradient the kernels implement."""
import contextlib
import io
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

import focal_ref as FR
import head_instances as HI
import tversky_ref as TR
from mliis_amd import args as A
from oracle import efficientlab_ref as R
from test_build_cpu import _affected_packed_forms, _dynamic_symbols

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "mliis_amd", "csrc")
NAMES = {"mliis_region_last_error", "mliis_tversky_ce_workspace_floats", "mliis_tversky_ce", "mliis_head_tversky_fused_supported",
         "mliis_head_tversky_fused_workspace_floats", "mliis_head_tversky_fused"}


def _quiet_stderr():
    return contextlib.redirect_stderr(io.StringIO())


# ------------------------------------------------------------------------------------------------ flags
def test_flag_becomes_a_learner_argument_and_is_absent_by_default():
    p, ref = A.argument_parser(), A.argument_parser(extensions=False)
    off = p.parse_args([])
    assert off.tversky is None and A.tversky(off) == {}
    for kw in (A.model_kwargs(off), A.model_kwargs(ref.parse_args([])), A.train_kwargs(off), A.evaluate_kwargs(off)):
        assert "tversky" not in kw
    on = A.model_kwargs(p.parse_args(["--tversky", "0.3", "0.7"]))
    assert on["tversky"] == (0.3, 0.7) and on["dice"] is False and "focal_gamma" not in on
    on = A.model_kwargs(p.parse_args(["--tversky", "1", "0", "--focal-gamma", "2", "--fg-weight", "4", "--loss_name", "bce_dice"]))
    assert on["tversky"] == (1.0, 0.0) and on["focal_gamma"] == 2.0 and on["fg_weight"] == 4.0 and on["dice"] is True
    assert A.model_kwargs(p.parse_args(["--tversky", "2", "0.25"]))["tversky"] == (2.0, 0.25)
    # the learner carries it: lanes, evaluation fine-tunes and the searches build their learners from model_kwargs
    assert "tversky" not in A.train_kwargs(p.parse_args(["--tversky", "0.3", "0.7"]))
    for bad in (["-1", "1"], ["1", "-0.5"], ["nan", "1"], ["1", "inf"], ["x", "1"], ["0", "0"], ["1"], []):
        with pytest.raises(SystemExit), _quiet_stderr():
            p.parse_args(["--tversky"] + bad)
    with pytest.raises(SystemExit), _quiet_stderr():                                   # the reference's parser has none
        ref.parse_args(["--tversky", "1", "1"])
    readme = open(os.path.join(ROOT, "README.md")).read()
    for text in (readme, p.format_help()):
        assert "--tversky" in text
    assert "Tversky" in readme and "Tversky" in open(os.path.join(ROOT, "DESIGN.md")).read()


def test_learner_refuses_bad_values_and_a_missing_library(monkeypatch, tmp_path):
    """Learner(tversky=(a, b)) loads the library in its constructor: a missing one fails there, loudly (the device check is stepped over:
    the refusal comes before any device work)."""
    import mliis_amd._lib as L
    from mliis_amd.learner import Learner
    monkeypatch.setattr(torch.cuda, "is_available", lambda: True)
    for bad in ((-1.0, 1.0), (1.0, -0.1), (float("nan"), 1.0), (1.0, float("inf")), (0.0, 0.0), (1.0,), (1.0, 1.0, 1.0), "ab", 0.5):
        with pytest.raises(ValueError, match="tversky"):
            Learner(image_size=64, tversky=bad)
    monkeypatch.setattr(L.region_lib, "_dll", None)
    monkeypatch.setattr(L.region_lib, "_path", str(tmp_path / "nope.so"))
    with pytest.raises(L.MliisError, match=r"nope\.so not found"):
        Learner(image_size=64, tversky=(0.3, 0.7))
    assert L.region_lib._dll is None


# ------------------------------------------------------------------------------------------------ the library
def _header_decls():
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "mliis_region.h")).read(), flags=re.S)
    return {m.group(1): [a for a in m.group(2).split(",") if a.strip() not in ("", "void")]
            for m in re.finditer(r"\b(mliis_\w+)\s*\(([^;{]*?)\)\s*;", src)}


def test_clean_out_of_tree_build_links_the_region_library(tmp_path):
    """A clean out-of-tree `make BUILD=... all` links the library: one translation unit built with -fno-slp-vectorize, the shared export
    map, exactly the header's names as dynamic symbols, a gfx950 code object only, none of the packed fp32 forms."""
    build = str(tmp_path / "obj")
    jobs = str(max(1, min(8, os.cpu_count() or 1)))
    r = subprocess.run(["make", "-C", CSRC, "-j" + jobs, "BUILD=" + build, "all"], capture_output=True, text=True, timeout=1500)
    assert r.returncode == 0, r.stderr[-3000:]
    so = os.path.join(build, "libmliis_region.so")
    assert os.path.exists(so) and os.path.exists(os.path.join(build, "tversky.o"))
    line = next(ln for ln in r.stdout.splitlines() if " tversky.hip " in ln + " ")
    assert "-fno-slp-vectorize" in line and "--offload-arch=gfx950" in line
    assert any("--version-script=exports.map" in ln and "libmliis_region.so" in ln for ln in r.stdout.splitlines())
    assert set(_dynamic_symbols(so)) == set(_header_decls()) == NAMES
    blob = open(so, "rb").read()
    assert b"gfx950" in blob and b"gfx942" not in blob and b"gfx90a" not in blob
    assert _affected_packed_forms(so) == {}
    mk = open(os.path.join(CSRC, "Makefile")).read()
    assert re.search(r"^all:.*\$\(REGION_TARGET\)", mk, flags=re.M) and re.search(r"rm -f .*\$\(REGION_OBJS\) \$\(REGION_TARGET\)", mk)
    assert re.search(r"^\$\(BUILD\)/tversky\.o:.*focal_math\.hpp.*loss_kernels\.hpp.*mliis_region\.h", mk, flags=re.M)


def test_region_library_exports_its_header_and_answers_without_a_gpu():
    from mliis_amd import _lib
    if not os.path.exists(_lib.REGION_LIB_PATH):
        import __graft_entry__ as g
        g.build()
    decls = _header_decls()
    assert set(decls) == set(_lib.REGION_SIGNATURES) == set(_dynamic_symbols(_lib.REGION_LIB_PATH)) == NAMES
    for name, params in decls.items():
        assert len(params) == len(_lib.REGION_SIGNATURES[name][1]), name
    assert not set(decls) & (set(_lib.SIGNATURES) | set(_lib.SCORE_SIGNATURES) | set(_lib.DATA_SIGNATURES) | set(_lib.STEPLOG_SIGNATURES) |
                             set(_lib.LAYERLOG_SIGNATURES) | set(_lib.CLIP_SIGNATURES) | set(_lib.SWEEP_SIGNATURES) | set(_lib.LOSS_SIGNATURES) |
                             set(_lib.TTA_SIGNATURES))
    assert _affected_packed_forms(_lib.REGION_LIB_PATH) == {}
    lib = _lib.region_lib
    dll = lib.load()
    # the workspace queries and the predicate: both entry points keep their partials per 2048-pixel block of the IMAGE
    for N, H, W in ((9, 9, 7), (17, 16, 12), (2, 257, 257), (1, 725, 725), (8, 224, 224)):
        assert lib.size("mliis_tversky_ce_workspace_floats", N, H, W) == HI.softmax_ce_workspace_floats(N, H, W)
        assert lib.size("mliis_head_tversky_fused_workspace_floats", N, 7, 5, H, W) == HI.softmax_ce_workspace_floats(N, H, W)
    for bad in ((0, 4, 4), (4, 0, 4), (4, 4, -1)):
        assert lib.size("mliis_tversky_ce_workspace_floats", *bad) == 0
        assert lib.size("mliis_head_tversky_fused_workspace_floats", bad[0], 4, 4, bad[1], bad[2]) == 0
        assert lib.size("mliis_head_tversky_fused_workspace_floats", 4, bad[1], bad[2], 8, 8) == (0 if bad[0] else HI.softmax_ce_workspace_floats(4, 8, 8))
    for c in TR.cases_of("head"):
        q = (c.p["Hd"], c.p["Wd"], c.p["H"], c.p["W"])
        assert bool(lib.size("mliis_head_tversky_fused_supported", *q)) == HI.head_supported(*q) == (c.inst != "refused"), c.name
    assert lib.size("mliis_head_tversky_fused_supported", 56, 56, 224, 224) == 1 and lib.size("mliis_head_tversky_fused_supported", 1, 8, 4, 32) == 0
    # the entry points refuse what they can without touching a device: nothing is launched for a null pointer or a bad value
    ce, head = dll.mliis_tversky_ce, dll.mliis_head_tversky_fused
    assert ce(None, None, None, 2, 4, 4, 0.0, 2.0, 4.0, 0.3, 0.7, 0.0, None, None, None, 1000, None) == -1
    assert dll.mliis_region_last_error().startswith(b"tversky_ce: null pointer")
    assert head(None, None, None, 2, 4, 4, 8, 8, 0.0, 2.0, 4.0, 0.3, 0.7, 0.0, None, None, None, 1000, None) == -1
    assert dll.mliis_region_last_error().startswith(b"head_tversky_fused: null pointer")
    # (a host buffer stands in for the device pointers: every check below fails before anything would be launched or dereferenced)
    host = np.zeros(4096, dtype=np.float32)
    ptr = host.ctypes.data + (-host.ctypes.data) % 16
    nan, inf = float("nan"), float("inf")
    for kw, word in ((dict(alpha=-0.5), b"alpha"), (dict(alpha=nan), b"alpha"), (dict(alpha=inf), b"alpha"), (dict(beta=-1.0), b"beta"),
                     (dict(beta=nan), b"beta"), (dict(beta=inf), b"beta"), (dict(alpha=0.0, beta=0.0), b"alpha + beta"),
                     (dict(gamma=-1.0), b"gamma"), (dict(gamma=nan), b"gamma"), (dict(gamma=inf), b"gamma"),
                     (dict(fgw=0.0), b"fg_weight"), (dict(fgw=-2.0), b"fg_weight"), (dict(fgw=nan), b"fg_weight"),
                     (dict(ls=1.0), b"label_smoothing"), (dict(ls=-0.1), b"label_smoothing"), (dict(ls=nan), b"label_smoothing"),
                     (dict(N=0), b"bad shape"), (dict(H=0), b"bad shape"), (dict(W=-3), b"bad shape"), (dict(ws=4), b"workspace")):
        a = dict(N=2, H=4, W=4, ls=0.0, gamma=2.0, fgw=4.0, alpha=0.3, beta=0.7, ws=1000)
        a.update(kw)
        assert ce(ptr, ptr, None, a["N"], a["H"], a["W"], a["ls"], a["gamma"], a["fgw"], a["alpha"], a["beta"], 0.0, ptr, ptr, ptr, a["ws"], None) < 0, kw
        assert word in dll.mliis_region_last_error(), (kw, dll.mliis_region_last_error())
        assert head(ptr, ptr, None, a["N"], a["H"], a["W"], 2 * a["H"], 2 * a["W"], a["ls"], a["gamma"], a["fgw"], a["alpha"], a["beta"], 0.0, ptr, ptr,
                    ptr, a["ws"], None) < 0, kw
        assert word in dll.mliis_region_last_error(), (kw, dll.mliis_region_last_error())
    # unaligned tensors and workspaces
    assert ce(ptr + 4, ptr, None, 2, 4, 4, 0.0, 0.0, 1.0, 1.0, 1.0, 0.0, ptr, ptr, ptr, 1000, None) == dll.mliis_tversky_ce(
        ptr, ptr + 4, None, 2, 4, 4, 0.0, 0.0, 1.0, 1.0, 1.0, 0.0, ptr, ptr, ptr, 1000, None) < 0
    assert b"8-byte aligned" in dll.mliis_region_last_error()
    assert head(ptr, ptr, None, 2, 4, 4, 8, 8, 0.0, 0.0, 1.0, 1.0, 1.0, 0.0, ptr + 4, ptr, ptr, 1000, None) < 0
    assert b"8-byte aligned" in dll.mliis_region_last_error()
    assert ce(ptr, ptr, None, 2, 4, 4, 0.0, 0.0, 1.0, 1.0, 1.0, 0.0, ptr, ptr, ptr + 8, 1000, None) < 0 and b"workspace" in dll.mliis_region_last_error()
    assert head(ptr, ptr, None, 2, 4, 4, 8, 8, 0.0, 0.0, 1.0, 1.0, 1.0, 0.0, ptr, ptr, ptr + 8, 1000, None) < 0 and b"workspace" in dll.mliis_region_last_error()
    assert head(ptr, ptr, None, 2, 11, 11, 49, 49, 0.0, 2.0, 4.0, 0.3, 0.7, 0.0, ptr, ptr, ptr, 100000, None) == -2
    assert b"up-sampling factor too large" in dll.mliis_region_last_error()
    assert not host.any()


def test_importing_the_package_or_building_a_plain_learner_does_not_load_the_region_library(monkeypatch):
    code = ("import mliis_amd, mliis_amd.ops, mliis_amd.learner, mliis_amd.reptile, mliis_amd._lib as L; assert L.region_lib._dll is None; "
            "assert L.loss_lib._dll is None; print('ok')")
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, cwd=ROOT, timeout=300)
    assert r.returncode == 0 and r.stdout.strip() == "ok", r.stderr[-2000:]
    # a learner without the argument gets as far as its first device work without touching the library (the device check is stepped over)
    import mliis_amd._lib as L
    from mliis_amd.learner import Learner
    monkeypatch.setattr(torch.cuda, "is_available", lambda: True)
    monkeypatch.setattr(L.region_lib, "_dll", None)
    monkeypatch.setattr(L.region_lib, "_path", str(os.path.join(ROOT, "no-such-dir", "nope.so")))
    with pytest.raises(Exception) as e:
        Learner(image_size=64, device="cuda:0")
    assert "nope.so" not in str(e.value) and L.region_lib._dll is None


# ------------------------------------------------------------------------------------------------ the reference
def test_case_list_spreads_the_pairs_and_shapes():
    ce, head = TR.cases_of("tversky_ce"), [c for c in TR.cases_of("head") if c.inst != "refused"]
    for group in (ce, head):
        assert {(c.p["alpha"], c.p["beta"]) for c in group} == set(TR.PAIRS)
        assert any((c.p["alpha"], c.p["beta"], c.p["gamma"], c.p["fgw"], c.p["ls"]) == (0.3, 0.7, 2.0, 4.0, 0.1) for c in group)
    assert {(c.p["N"], c.p["S"], c.p["H"], c.p["W"]) for c in ce} >= {(9, 4, 9, 7), (17, 17, 16, 12), (2, 2, 257, 257), (1, 1, 725, 725)}
    assert {c.inst for c in ce} == {TR.CHAIN, TR.CHAIN_NOGRAD} and any(c.p["zscale"] == 90.0 for c in ce) and any(c.p["extra"] for c in ce)
    assert {(c.p["Hd"], c.p["Wd"], c.p["H"], c.p["W"]) for c in head} == {(18, 11, 81, 48), (13, 7, 37, 28), (2, 2, 5, 5), (20, 9, 9, 39), (21, 21, 21, 21)}
    assert {(c.p["Hd"], c.p["Wd"], c.p["H"], c.p["W"]) for c in TR.cases_of("head") if c.inst == "refused"} == {(11, 11, 49, 49), (20, 9, 9, 40)}
    variants = [(c.p["Hd"], c.p["mask0"]) for c in head if c.p["mask0"]]
    assert sorted(variants) == [(13, "empty"), (13, "full"), (18, "empty"), (18, "full")]
    for c in head:
        if c.p["mask0"]:
            o = TR.head_oracle(c.name)
            assert o["used"][0, ..., 1].sum().item() == (0.0 if c.p["mask0"] == "empty" else c.p["H"] * c.p["W"])
    assert HI.softmax_ce_nblk(257, 257) == 33 and HI.softmax_ce_nblk(725, 725) == 256 and HI.cdiv(725 * 725, HI.CE_PIXELS_PER_BLOCK) > 256


@pytest.mark.parametrize("ls", [0.0, 0.1])
def test_reference_at_1_1_is_the_oracle_dice_loss(ls):
    """Value and gradient: alpha = beta = 1 on the plain pixel term is oracle.efficientlab_ref.loss_fn(dice=True)."""
    for seed, shape, zscale in ((1, (3, 9, 7, 2), 3.0), (2, (2, 16, 12, 2), 90.0)):
        z = (FR.rnd(*shape, seed=seed) * zscale).requires_grad_(True)
        y = FR.make_labels(shape[0], shape[1], shape[2], seed + 10, True)
        want = R.loss_fn(R.arch(), {}, z, y, ls, True, False)
        got, pix, iou = TR.loss_terms(z, y, ls, 0.0, 1.0, 1.0, 1.0)
        assert abs(got.item() - want.item()) <= 1e-12 * max(1.0, abs(want.item()))
        assert abs(iou.item() - TR.tversky_index(z, y, 1.0, 1.0).item()) <= 1e-15
        (gw,), (gg,) = torch.autograd.grad(want, [z]), torch.autograd.grad(got, [z])
        assert (gw - gg).abs().max().item() <= 1e-12 * gw.abs().max().item()
        # and alpha = beta = 1/2 is the soft Dice coefficient 2 I / (Sp + St)
        p1, y1 = torch.softmax(z, -1)[..., 1].flatten(1), y[..., 1].flatten(1)
        dice = ((2 * (p1 * y1).sum(1) + 2e-7) / (p1.sum(1) + y1.sum(1) + 2e-7)).mean()
        assert abs(TR.tversky_index(z, y, 0.5, 0.5).item() - dice.item()) <= 1e-12


@pytest.mark.parametrize("c", [c for c in TR.cases() if c.inst != "refused"], ids=TR.case_id)
def test_closed_form_gradient_equals_autograd(c):
    """The formula the kernels implement against autograd through the definition: 1e-12 of the largest entry, every pair, the saturated case
    and the empty / full masks included."""
    o = TR.ce_oracle(c.name) if c.entry == "tversky_ce" else TR.head_oracle(c.name)
    z = o["z"] if c.entry == "tversky_ce" else o["logits"]
    alpha, beta = FR.as_f32(c.p["alpha"]), FR.as_f32(c.p["beta"])
    mirror, auto = TR.region_grad_mirror(z.numpy(), o["used"].numpy(), alpha, beta), o["greg"].numpy()
    assert np.isfinite(mirror).all() and np.isfinite(auto).all() and np.abs(auto).max() > 0
    err = np.abs(mirror - auto).max() / np.abs(auto).max()
    print("tversky-figure | closed form vs autograd {} | {:.3e} | {:.1e}".format(c.name, err, 1e-12))
    assert err <= 1e-12
    assert np.array_equal(mirror[..., 0], -mirror[..., 1])
