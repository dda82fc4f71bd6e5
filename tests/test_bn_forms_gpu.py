"""Every instance of the batch-norm apply / backward kernels (bn.hip): each compile-time form the training passes reach, and the
run-time-flag instance through a flag combination no pass issues.

Reference: a float64 torch-CPU evaluation, at the tolerances of tests/test_ops_gpu.py::test_bn_train_fwd_bwd (statistics 1e-5, apply
2e-5, backward 1e-4, relative to the largest reference magnitude).  bf16 storage: the kernels compute in fp32 and round what they
store, so a stored value may sit one bf16 step (2^-7 of its magnitude at the most) from the rounded reference where the fp32 value
is near a tie; the bound is that step plus the fp32 tolerance.

Shapes are the smallest that reach every path: N = 2 / 3 images of 70 / 130 rows (a partial row batch; a 128-row pooling chunk that
ends inside an image), C = 4 / 24 / 40 / 112 (surplus channel lanes; more than one channel block), the 112 channels as a slice of a
224-wide buffer (ld > C: the decoder's concat), and 1 / 33 / 257 stage-1 partial blocks (one fold lane; one lane with two blocks;
more than one fold round)."""
import functools

import pytest
import torch

pytestmark = pytest.mark.gpu

BN_EPS = 1e-3
# (N, rows per image, C, wide: a slice of a 224-wide buffer, stage-1 partial blocks)
SHAPES = {"s1": (2, 70, 4, False, 1), "s2": (3, 130, 40, False, 33), "s3": (2, 130, 112, True, 257), "s4": (3, 70, 24, False, 33)}
SENTINEL = 7.0


def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


def rnd(*shape, seed=0):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed), dtype=torch.float64)


def swish(t):
    return t * torch.sigmoid(t)


def rel(got, ref):
    got, ref = got.detach().cpu().double(), ref.detach().cpu().double()
    assert got.shape == ref.shape, (got.shape, ref.shape)
    return (got - ref).abs().max().item() / max(ref.abs().max().item(), 1e-30)


def close(got, ref, tol, what):
    err = rel(got, ref)
    assert err <= tol, "{}: rel err {:.3e} > {:.1e}".format(what, err, tol)


def close_bf16(got, ref, tol, what):
    got, ref = got.detach().cpu().double(), ref.detach().cpu().double()
    bound = ref.abs() * 2.0 ** -7 + tol * ref.abs().max()
    bad = ((got - ref.to(torch.bfloat16).double()).abs() > bound).sum().item()
    assert bad == 0, "{}: {} values further than one bf16 step from the rounded reference".format(what, bad)


def put(t, d, wide=False, dtype=torch.float32):
    """t ([N, rows, 1, C], float64) on the device; wide: as channels 56..56+C of a 224-wide buffer filled with SENTINEL."""
    if not wide:
        return t.to(dtype).contiguous().to(d)
    buf = torch.full(t.shape[:-1] + (224,), SENTINEL, dtype=dtype, device=d)
    view = buf[..., 56:56 + t.shape[-1]]
    view.copy_(t.to(dtype))
    return view


def blank(shape, d, wide=False, dtype=torch.float32):
    return put(torch.full(shape, SENTINEL, dtype=torch.float64), d, wide, dtype)


def untouched(view, wide):
    """Nothing outside a wide slice was written."""
    if not wide:
        return True
    buf = view._base
    return bool((buf[..., :56] == SENTINEL).all() and (buf[..., 56 + view.shape[-1]:] == SENTINEL).all())


def partials(cols, nblk, d):
    """Stage-1 partial sums [nblk][len(cols)][C] (float32) of the row tensors in cols ([rows, C], float64): contiguous row chunks,
    empty ones where there are more blocks than rows."""
    rows = cols[0].shape[0]
    edges = [rows * k // nblk for k in range(nblk + 1)]
    part = torch.stack([torch.stack([c[edges[k]:edges[k + 1]].sum(0) for c in cols]) for k in range(nblk)])
    return part.float().contiguous().to(d)


@functools.lru_cache(maxsize=None)
def reference(shape, pre, post, isc, res, cs, ca, bf16, seed=0):
    """float64 forward and backward of one batch norm with the optional stages; bf16: the stored input / gradient are bf16 values."""
    N, rpi, C, _, _ = SHAPES[shape]
    q = (lambda t: t.to(torch.bfloat16).double()) if bf16 else (lambda t: t)
    x = q(rnd(N, rpi, 1, C, seed=seed + 14) * 2 + 0.5).requires_grad_(True)
    gamma = (rnd(C, seed=seed + 15) * 0.5 + 1).requires_grad_(True)
    beta = rnd(C, seed=seed + 16).requires_grad_(True)
    r = dict(x=x, gamma=gamma, beta=beta, resid=rnd(N, rpi, 1, C, seed=seed + 17), dy=q(rnd(N, rpi, 1, C, seed=seed + 22)),
             img_scale=torch.tensor([0.0, 1.25, 0.75][:N], dtype=torch.float64), chan_scale=rnd(N, C, seed=seed + 18),
             chan_add=rnd(N, C, seed=seed + 19) * 0.1, mm0=rnd(C, seed=seed + 20), mv0=rnd(C, seed=seed + 21).abs() + 0.5,
             skip0=rnd(N, rpi, 1, C, seed=seed + 23))
    xin = swish(x) if pre else x
    mean = xin.mean(dim=(0, 1, 2))
    var = ((xin - mean) ** 2).mean(dim=(0, 1, 2))
    xhat = (xin - mean) * torch.rsqrt(var + BN_EPS)
    u = xhat * gamma + beta
    out = swish(u) if post else u
    y = out
    if isc:
        y = y * r["img_scale"][:, None, None, None]
    if res:
        y = y + r["resid"]
    up = r["dy"]
    if isc:
        up = up * r["img_scale"][:, None, None, None]
    if cs:
        up = up * r["chan_scale"][:, None, None, :]
    if ca:
        up = up + r["chan_add"][:, None, None, :]
    gx, gg, gb = torch.autograd.grad(out, [x, gamma, beta], up)
    g = up * (torch.sigmoid(u) * (1 + u * (1 - torch.sigmoid(u)))) if post else up   # gradient at the affine output
    r.update(xin=xin.detach(), mean=mean.detach(), var=var.detach(), xhat=xhat.detach(), y=y.detach(), gx=gx, gg=gg, gb=gb, g=g.detach())
    r["x"], r["gamma"], r["beta"] = x.detach(), gamma.detach(), beta.detach()
    return r


# name -> (pre, post, isc, res, pool, bf16); "generic*": combinations no pass issues
APPLY_FORMS = {
    "post": (0, 1, 0, 0, 0, 0), "post_pool": (0, 1, 0, 0, 1, 0), "plain": (0, 0, 0, 0, 0, 0), "res": (0, 0, 0, 1, 0, 0),
    "isc_res": (0, 0, 1, 1, 0, 0), "pre": (1, 0, 0, 0, 0, 0), "pre_res": (1, 0, 0, 1, 0, 0), "generic_pre_post_isc": (1, 1, 1, 0, 0, 0),
    "generic_pool_res": (0, 0, 0, 1, 1, 0), "bf16_post": (0, 1, 0, 0, 0, 1), "bf16_post_pool": (0, 1, 0, 0, 1, 1),
    "bf16_generic_pre": (1, 0, 0, 0, 0, 1),
}


def _apply_once(ops, d, shape, form):
    pre, post, isc, res, pool, bf16 = APPLY_FORMS[form]
    N, rpi, C, wide, nblk = SHAPES[shape]
    R = reference(shape, pre, post, isc, res, 0, 0, bf16)
    dt = torch.bfloat16 if bf16 else torch.float32
    xg, y = put(R["x"], d, wide, dt), blank((N, rpi, 1, C), d, wide, dt)
    xin = R["xin"].reshape(-1, C)
    part = partials([xin, xin * xin], nblk, d)
    m, r_ = torch.empty(C, device=d), torch.empty(C, device=d)
    mm, mv = R["mm0"].float().to(d), R["mv0"].float().to(d)
    pool_part = torch.full((N * 4 * C + 16,), SENTINEL, device=d) if pool else None
    got = ops.bn_apply_fused(xg, part, nblk, m, r_, R["gamma"].float().to(d), R["beta"].float().to(d), moving=(mm, mv),
                             unbiased_moving_var=bool(pre), pre_swish=bool(pre), post_swish=bool(post),
                             img_scale=R["img_scale"].float().to(d) if isc else None, res=put(R["resid"], d, wide) if res else None, out=y,
                             pool_part=pool_part)
    chunks = got[1] if pool else 0
    return R, y, m, r_, mm, mv, pool_part, chunks


@pytest.mark.parametrize("shape", sorted(SHAPES))
@pytest.mark.parametrize("form", sorted(APPLY_FORMS))
def test_bn_apply_forms(form, shape):
    from mliis_amd import ops
    d = dev()
    pre, post, isc, res, pool, bf16 = APPLY_FORMS[form]
    N, rpi, C, wide, nblk = SHAPES[shape]
    R, y, m, r_, mm, mv, pool_part, chunks = _apply_once(ops, d, shape, form)
    n = N * rpi
    close(m, R["mean"], 1e-5, "mean")
    close(r_, torch.rsqrt(R["var"] + BN_EPS), 1e-5, "rstd")
    close(mm, R["mm0"] - (R["mm0"] - R["mean"]) * 0.01, 1e-5, "moving mean")
    close(mv, R["mv0"] - (R["mv0"] - R["var"] * (n / (n - 1.0) if pre else 1.0)) * 0.01, 1e-5, "moving var")
    (close_bf16 if bf16 else close)(y, R["y"], 2e-5, "apply")
    assert untouched(y, wide), "wrote outside the channel slice"
    if pool:
        assert chunks >= 1 and (pool_part[N * chunks * C:] == SENTINEL).all()
        sums = pool_part[:N * chunks * C].view(N, chunks, C).double().sum(1).cpu()
        stored = y.double().cpu()   # (the pooled sums are of the values the launch stored)
        close(sums, stored.sum(dim=(1, 2)), 1e-5, "pooled sums")
    again = _apply_once(ops, d, shape, form)
    for a, b in zip((y, m, r_, mm, mv), again[1:6]):
        assert torch.equal(a, b), "a second call returned other bits"
    if pool:
        assert torch.equal(pool_part, again[6])


@pytest.mark.parametrize("shape", sorted(SHAPES))
@pytest.mark.parametrize("pre,post", [(1, 0), (1, 1)])   # the decoder's pair, and the generic instance
def test_bn_apply_pair_forms(pre, post, shape):
    from mliis_amd import ops
    d = dev()
    N, rpi, C, wide, nblk = SHAPES[shape]
    Rs = [reference(shape, pre, post, 0, 0, 0, 0, 0, seed=s) for s in (0, 100)]

    def once():
        probs, outs = [], []
        for i, R in enumerate(Rs):
            xin = R["xin"].reshape(-1, C)
            nb = (nblk, max(1, nblk // 2))[i]   # (the two problems bring their own partial counts)
            y, m, r_ = blank((N, rpi, 1, C), d, wide), torch.empty(C, device=d), torch.empty(C, device=d)
            mm, mv = R["mm0"].float().to(d), R["mv0"].float().to(d)
            probs.append((put(R["x"], d, wide), partials([xin, xin * xin], nb, d), nb, m, r_, R["gamma"].float().to(d), R["beta"].float().to(d),
                          (mm, mv), y))
            outs.append((y, m, r_, mm, mv))
        ops.bn_apply_fused_pair(probs, pre_swish=bool(pre), post_swish=bool(post), unbiased_moving_var=True)
        return outs
    outs = once()
    n = N * rpi
    for R, (y, m, r_, mm, mv) in zip(Rs, outs):
        close(m, R["mean"], 1e-5, "mean")
        close(r_, torch.rsqrt(R["var"] + BN_EPS), 1e-5, "rstd")
        close(mm, R["mm0"] - (R["mm0"] - R["mean"]) * 0.01, 1e-5, "moving mean")
        close(mv, R["mv0"] - (R["mv0"] - R["var"] * n / (n - 1.0)) * 0.01, 1e-5, "moving var")
        close(y, R["y"], 2e-5, "pair apply")
        assert untouched(y, wide)
    for a, b in zip(outs, once()):
        assert all(torch.equal(s, t) for s, t in zip(a, b)), "a second call returned other bits"


# name -> (pre, post, is, cs, ca, skip: 0 none / 1 written / 2 accumulated, dxsum, bf16)
BWD_FORMS = {
    "pre": (1, 0, 0, 0, 0, 0, 0, 0), "pre_dxsum": (1, 0, 0, 0, 0, 0, 1, 0), "post": (0, 1, 0, 0, 0, 0, 0, 0), "plain": (0, 0, 0, 0, 0, 0, 0, 0),
    "skip_w": (0, 0, 0, 0, 0, 1, 0, 0), "skip_a": (0, 0, 0, 0, 0, 2, 0, 0), "is_skip_w": (0, 0, 1, 0, 0, 1, 0, 0), "is_skip_a": (0, 0, 1, 0, 0, 2, 0, 0),
    "post_cs_ca": (0, 1, 0, 1, 1, 0, 0, 0), "generic_all": (1, 1, 1, 1, 1, 2, 1, 0), "generic_post_skip_w": (0, 1, 0, 0, 0, 1, 0, 0),
    "bf16_post": (0, 1, 0, 0, 0, 0, 0, 1), "bf16_post_cs_ca": (0, 1, 0, 1, 1, 0, 0, 1), "bf16_generic_is": (0, 0, 1, 0, 0, 0, 0, 1),
}


def _bwd_once(ops, d, shape, form, stage1):
    pre, post, is_, cs, ca, skip, dxsum, bf16 = BWD_FORMS[form]
    N, rpi, C, wide, nblk = SHAPES[shape]
    R = reference(shape, pre, post, is_, 0, cs, ca, bf16)
    dt = torch.bfloat16 if bf16 else torch.float32
    f = lambda t: t.float().contiguous().to(d)   # noqa: E731
    dx = blank((N, rpi, 1, C), d, wide, dt)
    dg, db = torch.empty(C, device=d), torch.empty(C, device=d)
    sk = put(R["skip0"], d, wide) if skip else None
    slab = torch.full((ops.bn_bwd_dxsum_floats(N * rpi, C) + 8,), SENTINEL, device=d) if dxsum else None
    g, xhat = R["g"].reshape(-1, C), R["xhat"].reshape(-1, C)
    ops.bn_bwd(put(R["x"], d, wide, dt), put(R["dy"], d, wide, dt), f(R["mean"]), f(torch.rsqrt(R["var"] + BN_EPS)), f(R["gamma"]), f(R["beta"]),
               bool(pre), bool(post), f(R["img_scale"]) if is_ else None, f(R["chan_scale"]) if cs else None, f(R["chan_add"]) if ca else None,
               dx=dx, dgamma=dg, dbeta=db, dskip=sk, dskip_accumulate=skip == 2, dxsum_part=slab,
               stage1=(partials([g, g * xhat], nblk, d), nblk) if stage1 else None)
    return R, dx, dg, db, sk, slab


@pytest.mark.parametrize("stage1", [True, False])   # stage 1 from a producer (1 / 33 / 257 partial blocks), or the kernel's own reduce pass
@pytest.mark.parametrize("shape", sorted(SHAPES))
@pytest.mark.parametrize("form", sorted(BWD_FORMS))
def test_bn_bwd_forms(form, shape, stage1):
    from mliis_amd import ops
    d = dev()
    pre, post, is_, cs, ca, skip, dxsum, bf16 = BWD_FORMS[form]
    N, rpi, C, wide, nblk = SHAPES[shape]
    R, dx, dg, db, sk, slab = _bwd_once(ops, d, shape, form, stage1)
    (close_bf16 if bf16 else close)(dx, R["gx"], 1e-4, "dx")
    close(dg, R["gg"], 1e-4, "dgamma")
    close(db, R["gb"], 1e-4, "dbeta")
    assert untouched(dx, wide), "wrote outside the channel slice"
    if skip:
        close(sk, R["dy"] + R["skip0"] if skip == 2 else R["dy"], 1e-6, "skip gradient")
        assert untouched(sk, wide)
    if dxsum:
        nfl = slab.numel() - 8
        assert (slab[nfl:] == SENTINEL).all()
        got = slab[:nfl].view(-1, C).double().sum(0).cpu()
        scale = R["gx"].abs().sum(dim=(0, 1, 2)).max().item()   # (the true column sums can be ~0: compare on the sum's scale)
        assert (got - R["gx"].sum(dim=(0, 1, 2))).abs().max().item() <= 1e-5 * scale, "dx column sums"
    again = _bwd_once(ops, d, shape, form, stage1)
    for a, b in zip((dx, dg, db, sk, slab), again[1:]):
        assert a is None or torch.equal(a, b), "a second call returned other bits"


@pytest.mark.parametrize("shape", sorted(SHAPES))
@pytest.mark.parametrize("pre,post,dxsum", [(1, 0, 1), (1, 0, 0), (0, 1, 1)])   # the decoder's pair with / without the bias slabs; generic
def test_bn_bwd_pair_forms(pre, post, dxsum, shape):
    from mliis_amd import ops
    d = dev()
    N, rpi, C, wide, nblk = SHAPES[shape]
    Rs = [reference(shape, pre, post, 0, 0, 0, 0, 0, seed=s) for s in (0, 100)]
    f = lambda t: t.float().contiguous().to(d)   # noqa: E731
    nfl = ops.bn_bwd_dxsum_floats(N * rpi, C)

    def once():
        probs, outs = [], []
        for R in Rs:
            dx, dg, db = blank((N, rpi, 1, C), d, wide), torch.empty(C, device=d), torch.empty(C, device=d)
            slab = torch.full((nfl + 8,), SENTINEL, device=d) if dxsum else None
            probs.append((put(R["x"], d, wide), put(R["dy"], d, wide), f(R["mean"]), f(torch.rsqrt(R["var"] + BN_EPS)), f(R["gamma"]), f(R["beta"]),
                          dx, dg, db, slab))
            outs.append((dx, dg, db, slab))
        ops.bn_bwd_pair(probs, pre_swish=bool(pre), post_swish=bool(post))
        return outs
    outs = once()
    for R, (dx, dg, db, slab) in zip(Rs, outs):
        close(dx, R["gx"], 1e-4, "pair dx")
        close(dg, R["gg"], 1e-4, "pair dgamma")
        close(db, R["gb"], 1e-4, "pair dbeta")
        assert untouched(dx, wide)
        if dxsum:
            got = slab[:nfl].view(-1, C).double().sum(0).cpu()
            scale = R["gx"].abs().sum(dim=(0, 1, 2)).max().item()
            assert (got - R["gx"].sum(dim=(0, 1, 2))).abs().max().item() <= 1e-5 * scale, "pair dx column sums"
    for a, b in zip(outs, once()):
        assert all(s is None or torch.equal(s, t) for s, t in zip(a, b)), "a second call returned other bits"


@pytest.mark.parametrize("shape", sorted(SHAPES))
@pytest.mark.parametrize("bf16", [0, 1])
def test_se_bn_bwd_sums_and_stats_partial(bf16, shape):
    """The reduce passes whose loaders share the row addressing: the five per-image sums of the squeeze-excite backward (float and
    bf16 storage) and the stage-1 statistics (plain and of swish(x))."""
    from mliis_amd import ops
    d = dev()
    N, rpi, C, wide, _ = SHAPES[shape]
    R = reference(shape, 0, 1, 0, 0, 0, 0, bf16)
    dt = torch.bfloat16 if bf16 else torch.float32
    f = lambda t: t.float().contiguous().to(d)   # noqa: E731
    part = torch.full((ops.se_bn_bwd_sums_floats(N, rpi, C) + 8,), SENTINEL, device=d)
    args = (put(R["x"], d, wide, dt), put(R["dy"], d, wide, dt), f(R["mean"]), f(torch.rsqrt(R["var"] + BN_EPS)), f(R["gamma"]), f(R["beta"]))
    nb = ops.se_bn_bwd_sums(*args, part)
    u = R["xhat"] * R["gamma"] + R["beta"]
    sg = torch.sigmoid(u)
    dsw = sg * (1 + u * (1 - sg))
    want = torch.stack([R["dy"] * u * sg, R["dy"] * dsw, R["dy"] * dsw * R["xhat"], dsw, dsw * R["xhat"]], 1).sum(dim=(2, 3))   # [N, 5, C]
    got = part[:N * nb * 5 * C].view(N, nb, 5, C).double().sum(1).cpu()
    scale = torch.stack([R["dy"] * u * sg, R["dy"] * dsw, R["dy"] * dsw * R["xhat"], dsw, dsw * R["xhat"]], 1).abs().sum(dim=(2, 3)).max().item()
    assert (got - want).abs().max().item() <= 1e-5 * scale, "squeeze-excite / bn1 backward sums"
    assert (part[N * nb * 5 * C:] == SENTINEL).all()
    part2 = torch.full_like(part, SENTINEL)
    assert ops.se_bn_bwd_sums(*args, part2) == nb and torch.equal(part, part2), "a second call returned other bits"
    if bf16:
        return
    for pre in (False, True):
        sp = torch.full((ops.bn_stats_partial_floats(N * rpi, C) + 8,), SENTINEL, device=d)
        xg = put(R["x"], d, wide)
        nblk = ops.bn_stats_partial(xg, pre, sp)
        xin = (swish(R["x"]) if pre else R["x"]).reshape(-1, C)
        folded = sp[:nblk * 2 * C].view(nblk, 2, C).double().sum(0).cpu()
        close(folded[0], xin.sum(0), 1e-5, "sum")
        close(folded[1], (xin * xin).sum(0), 1e-5, "sum of squares")
        sp2 = torch.full_like(sp, SENTINEL)
        assert ops.bn_stats_partial(xg, pre, sp2) == nblk and torch.equal(sp, sp2)
