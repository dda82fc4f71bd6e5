"""Every split-product kernel instance (csrc/conv_x3.hip; manifest, planner mirror and shape search: tests/x3_instances.py) on the
device: float64 parity at the project's bars (forward 2e-5, backward-data and filter gradients 1e-4 of the tensor's max-abs), the
fix-up's extras on every tile width, bit-exact cases that pin each of the six term products, and bit-equal repeats.  The name query is
asserted before every launch; outputs and the whole workspace start as NaN, the workspace has exactly the size the library asks for,
and a guard band lies behind both.

The bit-exact cases are what sees a dropped or mis-paired term product: one lost product of the six moves a result by about 2^-17 of
one term, an order of magnitude below the parity bars.  They make every output the sum of ONE nonzero product and zeros, so the
float64 result rounded to fp32 is the only right answer:
  A terms: one-hot weights of 1.0 -- A's hi, mid and lo against B's hi; the output is the shifted input, bit for bit;
  B terms: one-hot activations of +-2^e -- A's hi against B's hi, mid and lo; the output is a scaled weight;
  mid x mid: values 2^e (1 + 2^-10) on both sides -- their product 2^(e+f) (1 + 2^-9 + 2^-20) needs the mid x mid term for its last bit.
Run with -s for the measured errors per instance."""
import collections
import math

import pytest
import torch

import x3_instances as X

pytestmark = pytest.mark.gpu

FWD_TOL, BWD_TOL, SUM_TOL = 2e-5, 1e-4, 1e-5
GUARD = 1024
NAN = float("nan")
ERRORS = collections.OrderedDict()   # (instance, kind) -> measured error of max-abs


def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


def relerr(got, ref):
    got, ref = got.detach().cpu().double(), ref.detach().cpu().double()
    assert got.shape == ref.shape, (got.shape, ref.shape)
    return ((got - ref).abs().max() / max(ref.abs().max().item(), 1e-30)).item()


def close(got, ref, tol, what):
    err = relerr(got, ref)
    print("{}: rel err {:.3e} (bar {:.1e})".format(what, err, tol))
    assert err <= tol, "{}: rel err {:.3e} > {:.1e}".format(what, err, tol)   # (a NaN left in the output fails here too)
    return err


class GuardedWs:
    """A workspace of exactly the floats the library asks for, NaN all over, with a guard band behind it (ops.Workspace's interface)."""

    def __init__(self, s, d):
        self.n = X.lib_workspace_floats(s)
        assert self.n == X.workspace_floats(X.plan_of(s))
        self.all = torch.full((self.n + GUARD,), NAN, device=d)
        self.all[self.n:] = 3.0
        self.buf = self.all[:self.n]

    def get(self, floats):
        assert floats == self.n
        return self.buf

    def check(self, what):
        assert (self.all[self.n:] == 3.0).all(), what + ": the guard band behind the workspace"


class Out:
    """The Nout columns [8, 8 + Nout) of a buffer with 12 more columns, filled with `fill`; 5.0 beside and behind them."""

    def __init__(self, s, d, fill=NAN):
        m, self.ld, self.nout = X.rows(s), s.Nout + 12, s.Nout
        self.flat = torch.full((m * self.ld + GUARD,), 5.0, device=d)
        self.full = self.flat[:m * self.ld].view(s.N, s.H, s.W, self.ld)
        self.view = self.full[..., 8:8 + s.Nout]
        if isinstance(fill, torch.Tensor):
            self.view.copy_(fill)
        else:
            self.view.fill_(fill)

    def check(self, what):
        assert (self.full[..., :8] == 5).all() and (self.full[..., 8 + self.nout:] == 5).all(), what + ": columns beside the output slice"
        assert (self.flat[self.full.numel():] == 5).all(), what + ": the guard band behind the output"


def launch(s, direction, a, image, d, fill=NAN, **kw):
    """One guarded call of the instance shape s is listed for; returns the Out."""
    from mliis_amd import ops
    nt = X.plan_of(s).nt
    what = "{} {}".format(X.conv_name(nt, direction), tuple(s))
    assert ops.conv2d_x3_kernel_name(s.N, s.H, s.W, s.Cred, s.Nout, s.ksize) == "conv_x3_k<%d>" % nt, what
    out, ws = Out(s, d, fill), GuardedWs(s, d)
    if direction == "fwd":
        r = ops.conv2d_fwd_x3(a, image, s.ksize, s.Nout, kw.pop("bias", None), s.dil, out=out.view, ws=ws, **kw)
    else:
        r = ops.conv2d_bwd_data_x3(a, image, s.ksize, s.Nout, s.dil, out=out.view, ws=ws, **kw)
    out.nblk = r[1] if isinstance(r, tuple) else None
    out.check(what)
    ws.check(what)
    return out


def weights_of(s, direction, w):
    """GEMM operand B [K = taps x Cred, Nout] -> the conv's weight tensor [k, k, Cin, Cout] (mode 1 images: B[n = ci][k = (tap, co)])."""
    k = s.ksize
    w = w.reshape(k, k, s.Cred, s.Nout)
    return w.contiguous() if direction == "fwd" else w.permute(0, 1, 3, 2).contiguous()


def reference(s, direction, a, w):
    return X.conv_ref(a, w, s.dil) if direction == "fwd" else X.bwd_data_ref(a, w, s.dil)


def operands(s, direction, seed):
    """(a, total weights with four more channels on either side of the window, the window's weights, float64 reference)."""
    g = torch.Generator().manual_seed(seed)
    a = torch.randn(s.N, s.H, s.W, s.Cred, generator=g)
    k, win = s.ksize, (s.Cred if direction == "fwd" else s.Nout)
    shape = (k, k, s.Cred + 8, s.Nout) if direction == "fwd" else (k, k, s.Nout + 8, s.Cred)
    wt = torch.randn(*shape, generator=g) / math.sqrt(X.kred(s))
    w = wt[:, :, 4:4 + win, :].contiguous()
    return a, wt, w, reference(s, direction, a, w)


def parity(s, direction, kind, seed):
    from mliis_amd import ops
    d = dev()
    nt = X.plan_of(s).nt
    a, _, w, ref = operands(s, direction, seed)
    ag, image = a.to(d), ops.x3_image_of(w.to(d), direction)
    out = launch(s, direction, ag, image, d)
    err = close(out.view, ref, FWD_TOL if direction == "fwd" else BWD_TOL, "{} {} {}".format(X.conv_name(nt, direction), kind, tuple(s)))
    ERRORS[(X.conv_name(nt, direction), kind, tuple(s))] = err
    again = launch(s, direction, ag, image, d)
    assert torch.equal(again.view, out.view), "{} {}: a second call differs".format(X.conv_name(nt, direction), tuple(s))
    return ag, image, out, ref


# ------------------------------------------------------------------------------------------------ parity and determinism
@pytest.mark.parametrize("direction", X.DIRECTIONS)
@pytest.mark.parametrize("nt", X.X3_NT)
def test_parity_of_every_instance_on_its_edge_and_loop_shape(nt, direction):
    for kind in X.KINDS:
        parity(X.searched()[(nt, direction, kind)], direction, kind, 100 + nt)


@pytest.mark.parametrize("direction", X.DIRECTIONS)
@pytest.mark.parametrize("case", range(len(X.FULL_TILE_CASES)))
def test_parity_on_one_whole_row_tile(case, direction):
    """NT 6 and 8 with all eight waves on valid rows (x3_instances.FULL_TILE_CASES: the searched shapes of these widths have 65 rows)."""
    parity(X.FULL_TILE_CASES[case], direction, "full", 200 + case)


def _with_border_bias(s, y, bb):
    """y [N, H, W, C] + bb [N, 9, C] by border class: (first row | interior | last row) x 3 + (first column | interior | last column)."""
    h = torch.arange(s.H).view(-1, 1).expand(s.H, s.W)
    w = torch.arange(s.W).view(1, -1).expand(s.H, s.W)
    hc = torch.where(h == 0, 0, torch.where(h == s.H - 1, 2, 1))
    wc = torch.where(w == 0, 0, torch.where(w == s.W - 1, 2, 1))
    cls = (hc * 3 + wc).reshape(-1)
    return y + bb.double()[:, cls, :].reshape(s.N, s.H, s.W, -1)


@pytest.mark.parametrize("direction", X.DIRECTIONS)
@pytest.mark.parametrize("case", range(len(X.CUT_CASES)))
def test_parity_of_the_stream_k_cut_cases(case, direction):
    """The cheap shapes that carry the cut classes (test_x3_instances_cpu.py says which case carries which), in both directions; the 3x3
    dilation-1 ones among them also with a border bias, on maps that have interior rows and columns."""
    s = X.CUT_CASES[case]
    ag, image, out, ref = parity(s, direction, "cut", 300 + case)
    if direction == "fwd" and s.ksize == 3 and s.dil == 1 and min(s.H, s.W) >= 2:
        d = dev()
        g = torch.Generator().manual_seed(400 + case)
        bias, bb = torch.randn(s.Nout, generator=g), torch.randn(s.N, 9, s.Nout, generator=g)
        o = launch(s, direction, ag, image, d, bias=bias.to(d), border_bias=bb.to(d))
        close(o.view, _with_border_bias(s, ref + bias.double(), bb), FWD_TOL, "cut case {} border bias".format(tuple(s)))


# ------------------------------------------------------------------------------------------------ the fix-up's extras, every tile width
def _stats_check(s, part, nblk, v, what):
    p = X.plan_of(s)
    assert nblk == X.FIX * p.gx, what
    blocks = part[: nblk * 2 * s.Nout].view(nblk, 2, s.Nout).double().cpu()
    assert (part[nblk * 2 * s.Nout:] == 7).all(), what + ": the partial buffer behind the blocks"
    close(blocks[:, 0].sum(0), v.sum(dim=(0, 1, 2)), SUM_TOL, what + ": fused sum")
    close(blocks[:, 1].sum(0), (v * v).sum(dim=(0, 1, 2)), SUM_TOL, what + ": fused sum of squares")
    # the 64-row quarters that lie wholly beyond the last row are written, as zeros; the others hold their own rows' sums
    flat = v.reshape(-1, s.Nout)
    for b in range(nblk):
        r0 = (b // X.FIX) * X.BM + (b % X.FIX) * (X.BM // X.FIX)
        own = flat[r0:r0 + X.BM // X.FIX]
        if own.shape[0] == 0:
            assert (blocks[b] == 0).all(), what + ": block {} lies beyond the rows".format(b)
        else:
            assert relerr(blocks[b, 0], own.sum(0)) <= 10 * SUM_TOL, what + ": block {}".format(b)


@pytest.mark.parametrize("nt", X.X3_NT)
def test_fixup_extras_forward(nt):
    """x3_fixup_k<NT> on the edge shape: bias; the fused statistics of the value and of swish(value); a border bias (the dilation-1
    variant of the shape -- the same plan; the edge maps have two rows: no interior row class); accumulate; and an input that is a
    channel window of a wider buffer, with the image packed for that window out of a wider weight tensor (NaN around both windows)."""
    from mliis_amd import ops
    d = dev()
    s = X.searched()[(nt, "fwd", "edge")]
    what = X.fixup_name(nt) + " " + str(tuple(s))
    a, wt, w, ref = operands(s, "fwd", 500 + nt)
    g = torch.Generator().manual_seed(600 + nt)
    bias, bb, base = torch.randn(s.Nout, generator=g), torch.randn(s.N, 9, s.Nout, generator=g), torch.randn(s.N, s.H, s.W, s.Nout, generator=g)
    ag, image, bg = a.to(d), ops.x3_image_of(w.to(d), "fwd"), bias.to(d)
    yb = ref + bias.double()
    plain = launch(s, "fwd", ag, image, d, bias=bg)
    close(plain.view, yb, FWD_TOL, what + " bias")
    for swish in (False, True):
        part = torch.full((X.FIX * X.plan_of(s).gx * 2 * s.Nout + 64,), 7.0, device=d)
        part[: -64] = NAN
        o = launch(s, "fwd", ag, image, d, bias=bg, stats_part=part, stats_swish=swish)
        assert torch.equal(o.view, plain.view), what + ": the statistics change the output"
        v = o.view.double().cpu()                      # (the sums are those of the values written)
        _stats_check(s, part, o.nblk, v * torch.sigmoid(v) if swish else v, what + " swish={}".format(swish))
    # accumulate onto a filled output, without bias
    o = launch(s, "fwd", ag, image, d, fill=base.to(d), accumulate=True)
    close(o.view, base.double() + ref, FWD_TOL, what + " accumulate")
    # border bias: 3x3, dilation 1
    s1 = s._replace(dil=1)
    assert s.ksize == 3 and s.H == 2 and X.plan_of(s1) == X.plan_of(s)
    o = launch(s1, "fwd", ag, image, d, bias=bg, border_bias=bb.to(d))
    close(o.view, _with_border_bias(s1, X.conv_ref(a, w, 1) + bias.double(), bb), FWD_TOL, what + " border bias")
    # the input as channels [4, 4 + Cred) of a wider buffer, the image packed for that window
    buf = torch.full((s.N, s.H, s.W, s.Cred + 8), NAN)
    buf[..., 4:4 + s.Cred] = a
    wn = torch.full_like(wt, NAN)
    wn[:, :, 4:4 + s.Cred, :] = w
    im = ops.X3Images(d)
    im.add("w", "fwd", 0, s.ksize, s.Cred + 8, s.Nout, 4, s.Cred)
    im.finish().pack(wn.to(d).view(-1))
    assert torch.equal(im.image("w", "fwd"), image), what + ": the window's image differs from the stand-alone one"
    o = launch(s, "fwd", buf.to(d)[..., 4:4 + s.Cred], im.image("w", "fwd"), d, bias=bg)
    assert torch.equal(o.view, plain.view), what + ": input window of a wider buffer"


@pytest.mark.parametrize("nt", X.X3_NT)
def test_fixup_extras_backward_data(nt):
    """Backward-data on the edge shape: accumulate into a channel slice of a filled gradient buffer, and dy as a channel window of a
    wider buffer against the image of the input-channel window [4, 4 + Nout) of a wider weight tensor (NaN around the windows)."""
    from mliis_amd import ops
    d = dev()
    s = X.searched()[(nt, "bwd", "edge")]
    what = X.fixup_name(nt) + " bwd " + str(tuple(s))
    a, wt, w, ref = operands(s, "bwd", 700 + nt)
    base = torch.randn(s.N, s.H, s.W, s.Nout, generator=torch.Generator().manual_seed(800 + nt))
    ag, image = a.to(d), ops.x3_image_of(w.to(d), "bwd")
    plain = launch(s, "bwd", ag, image, d)
    o = launch(s, "bwd", ag, image, d, fill=base.to(d), accumulate=True)
    close(o.view, base.double() + ref, BWD_TOL, what + " accumulate")
    wn = torch.full_like(wt, NAN)
    wn[:, :, 4:4 + s.Nout, :] = w
    im = ops.X3Images(d)
    im.add("w", "bwd", 0, s.ksize, s.Nout + 8, s.Cred, 4, s.Nout)
    im.finish().pack(wn.to(d).view(-1))
    assert torch.equal(im.image("w", "bwd"), image), what + ": the window's image differs from the stand-alone one"
    buf = torch.full((s.N, s.H, s.W, s.Cred + 8), NAN)
    buf[..., 4:4 + s.Cred] = a
    o = launch(s, "bwd", buf.to(d)[..., 4:4 + s.Cred], im.image("w", "bwd"), d)
    assert torch.equal(o.view, plain.view), what + ": dy window of a wider buffer"


# ------------------------------------------------------------------------------------------------ bit-exact cases
def _wide(shape, g, spread):
    """fp32 values with full 24-bit significands over a wide exponent range."""
    return torch.randn(*shape, generator=g) * torch.exp(torch.randn(*shape, generator=g) * spread)


def _pow2(n, g, lo=-12, hi=12):
    return torch.pow(2.0, torch.randint(lo, hi + 1, (n,), generator=g).float()) * (torch.randint(0, 2, (n,), generator=g).float() * 2 - 1)


def _one_hot_b(s, g, value):
    """B [K, Nout]: column n holds value[n] at one (tap, channel) pair; the pairs cycle through every tap and spread over all channels,
    the first and the very last k among them."""
    taps, K = s.ksize * s.ksize, X.kred(s)
    n = torch.arange(s.Nout)
    # (centre tap, its column and its row first: on a map of two rows or columns at dilation 2 no other tap is inside)
    tap = torch.tensor([4, 1, 7, 3, 5, 0, 8, 2, 6])[n % 9] if taps == 9 else n * 0
    c = (n * max(s.Cred // s.Nout, 1) + (n // taps) * 5) % s.Cred
    if s.Nout >= 12:
        c[0], tap[0] = 0, 0
        c[-1], tap[-1] = s.Cred - 1, taps - 1
    b = torch.zeros(K, s.Nout)
    b[tap * s.Cred + c, n] = value
    return b


def _exact(s, direction, a, b, what):
    from mliis_amd import ops
    d = dev()
    w = weights_of(s, direction, b)
    want = reference(s, direction, a, w).float()
    assert torch.isfinite(want).all() and (want != 0).any()
    image = ops.x3_image_of(w.to(d), direction)
    out = launch(s, direction, a.to(d), image, d)
    got = out.view.cpu()
    bad = (got != want).sum().item()
    assert torch.equal(got, want), "{}: {} of {} outputs differ from the one exact product (first: {})".format(
        what, bad, want.numel(), [(float(x), float(y)) for x, y in zip(got[got != want][:3], want[got != want][:3])])
    assert torch.equal(launch(s, direction, a.to(d), image, d).view.cpu(), got), what + ": a second call differs"


@pytest.mark.parametrize("direction", X.DIRECTIONS)
@pytest.mark.parametrize("nt", X.X3_NT)
def test_exact_a_terms_and_indexing(nt, direction):
    """One-hot weights of 1.0: the output is the shifted input (0.0 outside the border), bit for bit -- A's three terms against B's hi,
    the tap offsets and the channel walk; at dilation 1 and 2.  Then the mid x mid product: values 2^e (1 + 2^-10) on both sides."""
    edge = X.searched()[(nt, direction, "edge")]
    g = torch.Generator().manual_seed(900 + nt)
    a = _wide((edge.N, edge.H, edge.W, edge.Cred), g, 8.0)
    for dil in (1, 2):
        s = edge._replace(dil=dil)
        _exact(s, direction, a, _one_hot_b(s, g, 1.0), "{} {} one-hot weights".format(X.conv_name(nt, direction), tuple(s)))
    m = 1.0 + 2.0 ** -10
    am = (_pow2(a.numel(), g) * m).view_as(a)
    _exact(edge, direction, am, _one_hot_b(edge, g, _pow2(edge.Nout, g) * m), "{} {} mid x mid".format(X.conv_name(nt, direction), tuple(edge)))


def _one_hot_a(s, g):
    """a [N, H, W, Cred] with at most one nonzero (+-2^e) per pixel, on pixels so far apart that no output pixel sees two of them: every
    pixel for a 1x1 conv, a lattice of stride 3 dil for a 3x3 one.  Few K rows are touched: one or two pixels (times nine taps) on the
    two-row edge maps, 65 of 32740 rows on the 1x1 loop shapes of NT 6..9 -- their channels are scattered from the first chunk to the
    last, the very last row included, but this is no dense cover: a lost hi x mid or hi x lo product is seen, a weight-image plane
    misplaced at a few k positions is left to the parity cases."""
    m = X.rows(s)
    a = torch.zeros(m, s.Cred)
    pix = torch.arange(m)
    if s.ksize == 3:
        h, w = (pix // s.W) % s.H, pix % s.W
        st = 3 * s.dil
        pix = pix[(h % st == min(1, s.H - 1)) & (w % st == min(1, s.W - 1))]
    assert len(pix) >= 1
    c = (pix * max(s.Cred // m, 1) * 7 + 13) % s.Cred
    c[-1] = s.Cred - 1
    a[pix, c] = _pow2(len(pix), g)
    return a.view(s.N, s.H, s.W, s.Cred)


@pytest.mark.parametrize("direction", X.DIRECTIONS)
@pytest.mark.parametrize("nt", X.X3_NT)
def test_exact_b_terms(nt, direction):
    """One-hot activations of +-2^e against weights with full significands: y[m, co] = w[tap, c(m), co] 2^e exactly -- A's hi against B's
    three terms, through the weight image.  The 3x3 edge shape and the 1x1 loop shape."""
    for kind in X.KINDS:
        s = X.searched()[(nt, direction, kind)]
        g = torch.Generator().manual_seed(1000 + nt)
        _exact(s, direction, _one_hot_a(s, g), _wide((X.kred(s), s.Nout), g, 3.0), "{} {} one-hot activations".format(X.conv_name(nt, direction), tuple(s)))


# ------------------------------------------------------------------------------------------------ filter gradients
def _fold(partial, total):
    n = partial.numel() // total
    return partial[: n * total].view(n, total).double().sum(0)


def _filter_launch(s, xg, problems, d, precision="fp32x3"):
    """problems: dY tensors of one FilterBatch over the same x; returns the folded gradients [k, k, Cin, Cout] (float64, host)."""
    from mliis_amd import ops
    name = X.filter_instance(s)
    assert name is not None and X.filter_plan(s)[:3] == (2, int(name.split("<")[1][0]), int(name.endswith("multitap"))), (name, s)
    n = ops.lib.size("mliis_conv2d_bwd_filter_workspace_floats", s.N, s.H, s.W, s.Cin, s.Cout, s.ksize)
    total = s.ksize * s.ksize * s.Cin * s.Cout
    assert n == X.filter_plan(s)[5] * total
    fb = ops.FilterBatch(d)
    fb.X3_WIDE = s.wide
    slabs = []
    for dyg in problems:
        slabs.append(torch.full((n + GUARD,), NAN, device=d))
        slabs[-1][n:] = 3.0
        fb.add(xg, dyg, s.ksize, s.dil, slabs[-1][:n])
    fb.launch(precision)
    torch.cuda.synchronize()
    # the group mliis_conv2d_bwd_filter_batched hands to conv_filter_x3_batched_k: TMF 2, 4..8 column tiles, no x_scale; the 256-channel
    # table exists exactly for the 256 body.  (That the split-product kernel and not the fp32 instruction ran is not visible in the
    # table: test_filter_gradient_instances compares the slabs with those of an "fp32" launch, which must differ.)
    assert any(t[6] is not None for t in fb.tables) == name.endswith(" 256"), (name, s)
    assert all(t[3] == 2 and t[4] in X.FILTER_NT and t[5] == 0 for t in fb.tables), name
    assert all((b[n:] == 3.0).all() for b in slabs), name + ": the guard band behind the slabs"
    return [_fold(b[:n], total).view(s.ksize, s.ksize, s.Cin, s.Cout).cpu() for b in slabs]


FILTER_NAMES = [X.filter_name(nt, b) for nt in X.FILTER_NT for b in X.FILTER_BODIES]


@pytest.mark.parametrize("name", FILTER_NAMES)
def test_filter_gradient_instances(name):
    """FilterBatch.launch("fp32x3") on the shapes that launch this (NT, body): float64 autograd at 1e-4 with a second problem in the
    same grid, the slabs poisoned and folded in float64; then two bit-exact cases -- dY one-hot in the pixel per column against X with
    full significands (the slab sum is one shifted X value times +-2^e), and the roles swapped: on the cheapest shape and, for the
    multitap form, on the 12-channel one as well."""
    d = dev()
    shapes = X.search_filter()[name]
    for i, s in enumerate(shapes):
        g = torch.Generator().manual_seed(1100 + i)
        x, dy = torch.randn(s.N, s.H, s.W, s.Cin, generator=g), torch.randn(s.N, s.H, s.W, s.Cout, generator=g)
        gw = X.filter_grad_ref(x, dy, s.ksize, s.dil)
        ga, gb = _filter_launch(s, x.to(d), [dy.to(d), (dy * 0.5).to(d)], d)
        ERRORS[(name, "filt", tuple(s))] = close(ga, gw, BWD_TOL, "{} {}".format(name, tuple(s)))
        close(gb, 0.5 * gw, BWD_TOL, "{} {} second problem".format(name, tuple(s)))
        # a quiet fall-back to the fp32 instruction would pass everything here, the exact cases included (one product is exact there
        # too): its sums of random data round differently, so equal gradients mean the same kernel ran
        (gn,) = _filter_launch(s, x.to(d), [dy.to(d)], d, precision="fp32")
        close(gn, gw, BWD_TOL, "{} {} native".format(name, tuple(s)))
        assert not torch.equal(gn, ga), "{} {}: the fp32x3 launch gives the native instruction's bits".format(name, tuple(s))
    for s in [t for i, t in enumerate(shapes) if i == 0 or t.Cin == 12]:
        _filter_exact(name, s, d)


def _filter_exact(name, s, d):
    g = torch.Generator().manual_seed(1200)
    m = s.N * s.H * s.W
    xw, dw = _wide((s.N, s.H, s.W, s.Cin), g, 3.0), _wide((s.N, s.H, s.W, s.Cout), g, 3.0)
    dy1 = torch.zeros(m, s.Cout)
    co = torch.arange(s.Cout)
    dy1[(co * max(m // s.Cout, 1) + 3) % m, co] = _pow2(s.Cout, g)
    dy1 = dy1.view(s.N, s.H, s.W, s.Cout)
    x1 = torch.zeros(m, s.Cin)
    ci = torch.arange(s.Cin)
    x1[(ci * max(m // s.Cin, 1) + 5) % m, ci] = _pow2(s.Cin, g)
    x1 = x1.view(s.N, s.H, s.W, s.Cin)
    for what, xe, dye in (("one-hot dY", xw, dy1), ("one-hot X", x1, dw)):
        want = X.filter_grad_ref(xe, dye, s.ksize, s.dil).float()
        assert (want != 0).any()
        (got,) = _filter_launch(s, xe.to(d), [dye.to(d)], d)
        assert torch.equal(got.float(), want), "{} {} {}: {} of {} differ".format(name, tuple(s), what, (got.float() != want).sum().item(), want.numel())


def test_filter_batch_sends_other_channel_counts_to_the_native_instruction():
    """36, 100, 132 and 260 input channels plan 64-channel tiles (test_x3_instances_cpu.py): in one "fp32x3" batch with a problem that
    does take the split products they run the fp32 instruction, and every gradient is right."""
    from mliis_amd import ops
    d = dev()
    N, H, W, cout = 4, 30, 30, 52
    g = torch.Generator().manual_seed(1300)
    dy = torch.randn(N, H, W, cout, generator=g)
    fb, jobs = ops.FilterBatch(d), []
    for cin, k in ((196, 3), (36, 1), (100, 3), (132, 3), (260, 1)):
        s = X.FShape(N, H, W, cin, cout, k, 1, True)
        assert (X.filter_instance(s) is None) == (cin != 196)
        x = torch.randn(N, H, W, cin, generator=g)
        n = ops.lib.size("mliis_conv2d_bwd_filter_workspace_floats", N, H, W, cin, cout, k)
        slab = torch.full((n,), NAN, device=d)
        fb.add(x.to(d), dy.to(d), k, 1, slab)
        jobs.append((s, slab, X.filter_grad_ref(x, dy, k, 1)))
    fb.launch("fp32x3")
    torch.cuda.synchronize()
    for s, slab, gw in jobs:
        close(_fold(slab, s.ksize * s.ksize * s.Cin * cout).view(s.ksize, s.ksize, s.Cin, cout).cpu(), gw, BWD_TOL, "batch member {}".format(tuple(s)))


def test_the_measured_errors():
    """(Not a check of its own: the table of what the parity tests above measured, for -s.)"""
    for (name, kind, s), err in ERRORS.items():
        print("{:22s} {:5s} {:38s} {:.2e}".format(name, kind, str(s), err))
