"""The focal, foreground-weighted pixel loss, the host half: the flags and the Learner arguments they become, libmliis_loss.so's build and
exported ABI against include/mliis_loss.h, its host-only queries and refusals, and the reference of tests/focal_ref.py against the
oracle's loss (gamma = 0, W = 1) and against the closed-form gradient the kernels implement."""
import contextlib
import io
import os
import re
import subprocess

import numpy as np
import pytest
import torch

import focal_ref as FR
import head_instances as HI
from mliis_amd import args as A
from oracle import efficientlab_ref as R
from test_build_cpu import _affected_packed_forms, _dynamic_symbols

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "mliis_amd", "csrc")
NAMES = {"mliis_loss_last_error", "mliis_focal_ce_workspace_floats", "mliis_focal_ce", "mliis_head_focal_fused_supported",
         "mliis_head_focal_fused_workspace_floats", "mliis_head_focal_fused"}


def _quiet_stderr():
    return contextlib.redirect_stderr(io.StringIO())


# ------------------------------------------------------------------------------------------------ flags
def test_flags_become_learner_arguments_and_are_absent_by_default():
    p, ref = A.argument_parser(), A.argument_parser(extensions=False)
    off = p.parse_args([])
    assert off.focal_gamma is None and off.fg_weight is None and A.focal_loss(off) == {}
    for kw in (A.model_kwargs(off), A.model_kwargs(ref.parse_args([])), A.train_kwargs(off), A.evaluate_kwargs(off)):
        assert not any("focal" in k or "fg_weight" in k for k in kw)
    on = A.model_kwargs(p.parse_args(["--focal-gamma", "2", "--fg-weight", "4"]))
    assert on["focal_gamma"] == 2.0 and on["fg_weight"] == 4.0
    on = A.model_kwargs(p.parse_args(["--focal-gamma", "0.5"]))
    assert on["focal_gamma"] == 0.5 and "fg_weight" not in on
    on = A.model_kwargs(p.parse_args(["--fg-weight", "0.25", "--loss_name", "bce_dice", "--inner-clip-norm", "1"]))
    assert on["fg_weight"] == 0.25 and "focal_gamma" not in on and on["dice"] is True and on["grad_clip"] == ("norm", 1.0)
    assert A.model_kwargs(p.parse_args(["--focal-gamma", "0"]))["focal_gamma"] == 0.0      # given, and the cross-entropy
    # the learner carries them: lanes, evaluation fine-tunes and the searches build their learners from model_kwargs
    assert not any("focal" in k or "fg_weight" in k for k in A.train_kwargs(p.parse_args(["--focal-gamma", "2", "--fg-weight", "4"])))
    for flag, bads in (("--focal-gamma", ("-1", "nan", "inf", "-0.5", "x")), ("--fg-weight", ("0", "-1", "nan", "inf", "x"))):
        for bad in bads:
            with pytest.raises(SystemExit), _quiet_stderr():
                p.parse_args([flag, bad])
        with pytest.raises(SystemExit), _quiet_stderr():                                   # the reference's parser has none
            ref.parse_args([flag, "1"])
    readme = open(os.path.join(ROOT, "README.md")).read()
    for text in (readme, p.format_help()):
        assert "--focal-gamma" in text and "--fg-weight" in text
    flat = re.sub(r"\s+", " ", readme)
    assert "focal pixel term" in flat and "N·H·W" in flat


def test_learner_refuses_bad_values_and_a_missing_library(monkeypatch, tmp_path):
    """Learner(focal_gamma=2.0) loads the library in its constructor: a missing one fails there, loudly (the device check is stepped over:
    the refusal comes before any device work)."""
    import mliis_amd._lib as L
    from mliis_amd.learner import Learner
    monkeypatch.setattr(torch.cuda, "is_available", lambda: True)
    for bad in (dict(focal_gamma=-1.0), dict(focal_gamma=float("nan")), dict(fg_weight=0.0), dict(fg_weight=float("inf"))):
        with pytest.raises(ValueError, match="focal_gamma|fg_weight"):
            Learner(image_size=64, **bad)
    monkeypatch.setattr(L.loss_lib, "_dll", None)
    monkeypatch.setattr(L.loss_lib, "_path", str(tmp_path / "nope.so"))
    for kw in (dict(focal_gamma=2.0), dict(fg_weight=4.0)):
        with pytest.raises(L.MliisError, match=r"nope\.so not found"):
            Learner(image_size=64, **kw)
    assert L.loss_lib._dll is None


# ------------------------------------------------------------------------------------------------ the library
def _header_decls():
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "mliis_loss.h")).read(), flags=re.S)
    return {m.group(1): [a for a in m.group(2).split(",") if a.strip() not in ("", "void")]
            for m in re.finditer(r"\b(mliis_\w+)\s*\(([^;{]*?)\)\s*;", src)}


def test_clean_out_of_tree_build_links_the_loss_library(tmp_path):
    """A clean out-of-tree `make BUILD=... all` links the library: one translation unit built with -fno-slp-vectorize, the shared export
    map, exactly the header's names as dynamic symbols, a gfx950 code object only, none of the packed fp32 forms."""
    build = str(tmp_path / "obj")
    jobs = str(max(1, min(8, os.cpu_count() or 1)))
    r = subprocess.run(["make", "-C", CSRC, "-j" + jobs, "BUILD=" + build, "all"], capture_output=True, text=True, timeout=1500)
    assert r.returncode == 0, r.stderr[-3000:]
    so = os.path.join(build, "libmliis_loss.so")
    assert os.path.exists(so) and os.path.exists(os.path.join(build, "focal.o"))
    line = next(ln for ln in r.stdout.splitlines() if " focal.hip " in ln + " ")
    assert "-fno-slp-vectorize" in line and "--offload-arch=gfx950" in line
    assert any("--version-script=exports.map" in ln and "libmliis_loss.so" in ln for ln in r.stdout.splitlines())
    assert set(_dynamic_symbols(so)) == set(_header_decls()) == NAMES
    blob = open(so, "rb").read()
    assert b"gfx950" in blob and b"gfx942" not in blob and b"gfx90a" not in blob
    assert _affected_packed_forms(so) == {}
    mk = open(os.path.join(CSRC, "Makefile")).read()
    assert re.search(r"^all:.*\$\(LOSS_TARGET\)", mk, flags=re.M) and re.search(r"rm -f .*\$\(LOSS_OBJS\) \$\(LOSS_TARGET\)", mk)


def test_loss_library_exports_its_header_and_answers_without_a_gpu():
    from mliis_amd import _lib
    if not os.path.exists(_lib.LOSS_LIB_PATH):
        import __graft_entry__ as g
        g.build()
    decls = _header_decls()
    assert set(decls) == set(_lib.LOSS_SIGNATURES) == set(_dynamic_symbols(_lib.LOSS_LIB_PATH)) == NAMES
    for name, params in decls.items():
        assert len(params) == len(_lib.LOSS_SIGNATURES[name][1]), name
    assert not set(decls) & (set(_lib.SIGNATURES) | set(_lib.SCORE_SIGNATURES) | set(_lib.DATA_SIGNATURES) | set(_lib.STEPLOG_SIGNATURES) |
                             set(_lib.LAYERLOG_SIGNATURES) | set(_lib.CLIP_SIGNATURES) | set(_lib.SWEEP_SIGNATURES))
    assert _affected_packed_forms(_lib.LOSS_LIB_PATH) == {}
    lib = _lib.loss_lib
    dll = lib.load()
    # the workspace queries and the predicate: head.hip's, which tests/head_instances.py mirrors
    for N, H, W in ((9, 9, 7), (17, 16, 12), (2, 257, 257), (1, 725, 725), (8, 224, 224)):
        assert lib.size("mliis_focal_ce_workspace_floats", N, H, W) == HI.softmax_ce_workspace_floats(N, H, W)
    for N, Hd, Wd in ((2, 18, 11), (9, 13, 7), (2, 2, 2), (8, 56, 56)):
        assert lib.size("mliis_head_focal_fused_workspace_floats", N, Hd, Wd) == HI.head_workspace_floats(N, Hd, Wd)
    for bad in ((0, 4, 4), (4, 0, 4), (4, 4, -1)):
        assert lib.size("mliis_focal_ce_workspace_floats", *bad) == 0 and lib.size("mliis_head_focal_fused_workspace_floats", *bad) == 0
    for c in FR.cases_of("head"):
        q = (c.p["Hd"], c.p["Wd"], c.p["H"], c.p["W"])
        assert bool(lib.size("mliis_head_focal_fused_supported", *q)) == HI.head_supported(*q) == (c.inst != "refused"), c.name
    assert lib.size("mliis_head_focal_fused_supported", 56, 56, 224, 224) == 1 and lib.size("mliis_head_focal_fused_supported", 1, 8, 4, 32) == 0
    # the entry points refuse what they can without touching a device: nothing is launched for a null pointer or a bad value
    ce, head = dll.mliis_focal_ce, dll.mliis_head_focal_fused
    assert ce(None, None, None, 2, 4, 4, 0.0, 2.0, 4.0, 0, 0.0, None, None, None, 1000, None) == -1
    assert dll.mliis_loss_last_error().startswith(b"focal_ce: null pointer")
    assert head(None, None, None, 2, 4, 4, 8, 8, 0.0, 2.0, 4.0, 0.0, None, None, None, 1000, None) == -1
    assert dll.mliis_loss_last_error().startswith(b"head_focal_fused: null pointer")
    # (a host buffer stands in for the device pointers: every check below fails before anything would be launched or dereferenced)
    host = np.zeros(4096, dtype=np.float32)
    ptr = host.ctypes.data + (-host.ctypes.data) % 16
    for kw, word in ((dict(gamma=-1.0), b"gamma"), (dict(gamma=float("nan")), b"gamma"), (dict(gamma=float("inf")), b"gamma"),
                     (dict(fgw=0.0), b"fg_weight"), (dict(fgw=-2.0), b"fg_weight"), (dict(fgw=float("nan")), b"fg_weight"),
                     (dict(ls=1.0), b"label_smoothing"), (dict(ls=-0.1), b"label_smoothing"), (dict(ls=float("nan")), b"label_smoothing"),
                     (dict(N=0), b"bad shape"), (dict(H=0), b"bad shape"), (dict(W=-3), b"bad shape"), (dict(ws=4), b"workspace")):
        a = dict(N=2, H=4, W=4, ls=0.0, gamma=2.0, fgw=4.0, ws=1000)
        a.update(kw)
        assert ce(ptr, ptr, None, a["N"], a["H"], a["W"], a["ls"], a["gamma"], a["fgw"], 0, 0.0, ptr, ptr, ptr, a["ws"], None) < 0, kw
        assert word in dll.mliis_loss_last_error(), (kw, dll.mliis_loss_last_error())
        assert head(ptr, ptr, None, a["N"], a["H"], a["W"], 2 * a["H"], 2 * a["W"], a["ls"], a["gamma"], a["fgw"], 0.0, ptr, ptr, ptr, a["ws"], None) < 0, kw
        assert word in dll.mliis_loss_last_error(), (kw, dll.mliis_loss_last_error())
    assert head(ptr, ptr, None, 2, 11, 11, 49, 49, 0.0, 2.0, 4.0, 0.0, ptr, ptr, ptr, 1000, None) == -2
    assert b"up-sampling factor too large" in dll.mliis_loss_last_error()
    assert not host.any()


def test_importing_the_package_does_not_load_the_loss_library():
    code = "import mliis_amd, mliis_amd.ops, mliis_amd.learner, mliis_amd.reptile, mliis_amd._lib as L; assert L.loss_lib._dll is None; print('ok')"
    import sys
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, cwd=ROOT, timeout=300)
    assert r.returncode == 0 and r.stdout.strip() == "ok", r.stderr[-2000:]


# ------------------------------------------------------------------------------------------------ the reference
def test_case_list_spreads_the_parameters():
    ce, head = FR.cases_of("focal_ce"), [c for c in FR.cases_of("head") if c.inst != "refused"]
    with_dice, without = [c.p for c in ce if c.p["dice"]], [c.p for c in ce if not c.p["dice"]] + [c.p for c in head]
    for group in (with_dice, without):
        assert {p["gamma"] for p in group} == set(FR.GAMMAS) and {p["fgw"] for p in group} == set(FR.WEIGHTS)
        assert {p["ls"] for p in group} == set(FR.SMOOTHINGS)
    forms = {c.inst for c in FR.cases() if (c.p["gamma"], c.p["fgw"]) == (2.0, 4.0)}
    assert forms == {FR.MERGED, FR.FOLD_ONLY, FR.THREE, ("head", "fold"), "refused"}
    assert {(c.p["N"], c.p["S"], c.p["H"], c.p["W"]) for c in ce} >= {(9, 4, 9, 7), (17, 17, 16, 12), (2, 2, 257, 257), (1, 1, 725, 725)}
    assert {(c.p["Hd"], c.p["Wd"], c.p["H"], c.p["W"]) for c in FR.cases_of("head")} == {
        (18, 11, 81, 48), (13, 7, 37, 28), (2, 2, 5, 5), (20, 9, 9, 39), (21, 21, 21, 21), (11, 11, 49, 49), (20, 9, 9, 40)}
    assert HI.softmax_ce_nblk(257, 257) == 33 and HI.softmax_ce_nblk(725, 725) == 256 and HI.cdiv(725 * 725, HI.CE_PIXELS_PER_BLOCK) > 256


@pytest.mark.parametrize("dice", [False, True])
@pytest.mark.parametrize("ls", [0.0, 0.1])
def test_reference_at_gamma_0_weight_1_is_the_oracle_loss(dice, ls):
    for seed, shape, zscale in ((1, (3, 9, 7, 2), 3.0), (2, (2, 16, 12, 2), 90.0)):
        z = FR.rnd(*shape, seed=seed) * zscale
        y = FR.make_labels(shape[0], shape[1], shape[2], seed + 10, True)
        want = R.loss_fn(R.arch(), {}, z, y, ls, dice, False)
        got, pix, iou = FR.loss_terms(z, y, ls, 0.0, 1.0, dice)
        assert abs(got.item() - want.item()) <= 1e-12 * max(1.0, abs(want.item()))
        assert abs(pix.item() - R.loss_fn(R.arch(), {}, z, y, ls, False, False).item()) <= 1e-12 * max(1.0, abs(pix.item()))


@pytest.mark.parametrize("c", [c for c in FR.cases() if c.inst != "refused"], ids=FR.case_id)
def test_closed_form_gradient_equals_autograd(c):
    """The formula the kernels implement against autograd through the definition: 1e-12 of the largest entry, the saturated cases included."""
    o = FR.ce_oracle(c.name) if c.entry == "focal_ce" else FR.head_oracle(c.name)
    z = o["z"] if c.entry == "focal_ce" else o["logits"]
    ls, gamma, fgw = (FR.as_f32(c.p[k]) for k in ("ls", "gamma", "fgw"))
    mirror, auto = FR.grad_mirror(z.numpy(), o["used"].numpy(), ls, gamma, fgw), o["gpix"].numpy()
    assert np.isfinite(mirror).all() and np.isfinite(auto).all()
    err = np.abs(mirror - auto).max() / np.abs(auto).max()
    print("focal-figure | closed form vs autograd {} | {:.3e} | {:.1e}".format(c.name, err, 1e-12))
    assert err <= 1e-12
    assert np.array_equal(mirror[..., 0], -mirror[..., 1])
