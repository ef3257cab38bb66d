"""cine_casorati_gram, cine_svt_weight and cine_ls_prox through the C ABI, shape by shape against tests/ls_reference.py in float64, with the
kernel_sweep harness: guarded outputs, an exact-size workspace with a sentinel tail, two calls with equal bits, refusals that write nothing.

Frames t: 2, 5, 15, 16, 64.  Pixels h * w: 1, and P - 1, P, P + 1, 2 P + 3 around each kernel's own pixel tile: P = cine_casorati_gram_pixels(t)
= 2048 // t for the Gram matrix, P = cine_ls_prox_pixels() = 64 for the prox.  Batch 2 once.

Bars.  Gram matrix of `a` alone: 1e-12 of max |G| against float64 numpy on the same float32 inputs (the products are exact, the sums float64);
with g: kernel_sweep.BAR = 1e-5, because v = a - step g is rounded to float32.  Bitwise Hermitian, a real diagonal.
Weight: W is not unique on the null space of G, so it is judged by its action, max |G^{1/2} (W - W_ref)| / sigma_max <= BAR with G^{1/2} and W_ref
from numpy.linalg.eigh; above sigma_max W is exactly zero; sigma_max within 1e-10 relative; residual <= 1e-14; sweeps below the cap.  The
nuclear norm sum_i sqrt(lam_i) h(lam_i) within 1e-10 relative PLUS the reference's own uncertainty: eigh returns the eigenvalues of a matrix
within t eps lam_max of G (Weyl), and sqrt turns that into sqrt(t eps lam_max) ~ 1e-7 sigma_max per eigenvalue near zero -- so for the rank-3
matrix and the 16-decade spectrum at threshold 0 no two eigensolvers agree to 1e-10, and NUC_UNCERTAINTY() adds what that costs.  For every
other case the term is below 1e-12 of the norm (asserted), a hundredth of the bar, and the bar is the plain 1e-10.  Measured on the MI355X: rank 3,
t = 64, threshold 0: 8.7e-8 of 2.61 apart with the reference uncertain by 7.3e-6; every well-posed case within 2e-15.
Prox: lnew, snew, xsum within BAR of the float64 peak (both proxes are 1-Lipschitz, so no margin round a kink is needed), the yardstick's
lnew from numpy.linalg.svd; the three sums within SUM_REL = 1e-4 relative, the bar the k-t sums hold."""
import numpy as np
import pytest
import torch

import kt_reference as R
import ls_reference as LS
from conftest import rnd
from kernel_sweep import BAR, EINVAL, EUNSUPPORTED, EWORKSPACE, Call, L, check, ptr, refused, same_bits, stream, twice

pytestmark = pytest.mark.gpu
SUM_REL = 1e-4
STEP = 0.45
FRAMES = [2, 5, 15, 16, 64]
KINDS = ["1", "P-1", "P", "P+1", "2P+3"]
MAX_SWEEPS = 40


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "-m gpu tests need an MI355X"
    return torch.device("cuda:0")


def pixels(kind, P):
    return {"1": 1, "P-1": P - 1, "P": P, "P+1": P + 1, "2P+3": 2 * P + 3}[kind]


def f64(t):
    """A float32 CPU tensor holding double pairs -> float64 numpy."""
    return t.contiguous().view(torch.float64).numpy()


def test_the_tiles_the_pixel_sizes_sit_around(dev):
    from cine_hip import ops
    assert ops.ls_prox_pixels() == 64 == L().cine_ls_prox_pixels()
    assert [L().cine_casorati_gram_pixels(t) for t in FRAMES] == [2048 // t for t in FRAMES]
    assert L().cine_casorati_gram_pixels(1) == 0 and L().cine_casorati_gram_pixels(65) == 0
    assert L().cine_ls_prox_ws_bytes(2, 5, 5, 13) == 2 * 2 * 16 and L().cine_ls_prox_ws_bytes(0, 5, 5, 13) == 0
    # the partial sums of the Gram matrix stay modest: one (t (t + 1) / 2) record of double pairs per workgroup, 256 workgroups at most
    assert L().cine_casorati_gram_ws_bytes(1, 64, 200, 200) == 250 * 2080 * 16 <= 256 * 2080 * 16            # 1250 tiles, 5 per workgroup
    assert L().cine_casorati_gram_ws_bytes(1, 64, 1, 33) == 2 * 2080 * 16
    assert L().cine_casorati_gram_ws_bytes(2, 15, 200, 200) == 2 * 99 * 120 * 16                              # 295 tiles, 3 per workgroup, 128 at most


# ------------------------------------------------------------------ the Gram matrix
def gram_call(k, a, g, shape):
    b, t, h, w = shape
    ai, gi = k.inp(a), k.inp(g)
    si = k.raw(torch.tensor([STEP])) if g is not None else None
    out = k.out((b, t, t, 4))                                  # double pairs, seen as floats by the guard
    nbytes = L().cine_casorati_gram_ws_bytes(b, t, h, w)
    ws = k.ws(nbytes)
    check(L().cine_casorati_gram(ptr(ai), ptr(gi), ptr(si), out.ptr(), b, t, h, w, ws.ptr(), nbytes, stream()), "cine_casorati_gram")
    return [out.t]


def check_gram(dev, shape, seed):
    b, t, h, w = shape
    a, g = rnd(seed, b, t, h, w, 2), rnd(seed + 1, b, t, h, w, 2)
    for with_g in (False, True):
        what = f"cine_casorati_gram {shape} g {int(with_g)}"
        (got,) = twice(dev, 0, lambda k: gram_call(k, a, g if with_g else None, shape), what)
        got = f64(got).reshape(b, t, t, 2)
        got = got[..., 0] + 1j * got[..., 1]
        v = R.to_complex(a) - (float(np.float32(STEP)) * R.to_complex(g) if with_g else 0.0)
        want = LS.gram(v)
        err = float(np.abs(got - want).max() / np.abs(want).max())
        bar = BAR if with_g else 1e-12
        print(f"{what}: {err:.2e} of max |G| (bar {bar:.0e})")
        assert err <= bar, what
        assert np.array_equal(got, np.conj(np.swapaxes(got, 1, 2))), what + ": not bitwise Hermitian"
        assert not np.diagonal(got, axis1=1, axis2=2).imag.any(), what + ": the diagonal is not real"


@pytest.mark.parametrize("kind", KINDS, ids=lambda p: f"pix{p}")
@pytest.mark.parametrize("t", FRAMES, ids=lambda t: f"t{t}")
def test_gram_vs_float64(dev, t, kind):
    n = pixels(kind, 2048 // t)
    check_gram(dev, (1, t, n, 1) if kind == "P+1" else (1, t, 1, n), seed=1000 * t + n)


def test_gram_vs_float64_batch_two(dev):
    check_gram(dev, (2, 5, 31, 27), seed=71)                   # 837 pixels: three tiles of 409, a record each


# ------------------------------------------------------------------ the weight
def gram_matrices(t, seed=0):
    """Six (t, t) Hermitian positive semidefinite matrices scaled to lam_max = 1 (the zero matrix apart), made in float64 on the host."""
    rs = np.random.RandomState(seed + t)

    def cn(*s):
        return rs.standard_normal(s) + 1j * rs.standard_normal(s)
    q, _ = np.linalg.qr(cn(t, t))
    x = cn(4 * t + 3, t)
    lo = cn(4 * t + 3, min(3, t)) @ cn(min(3, t), t)
    out = {"full rank": x.conj().T @ x, "rank 3": lo.conj().T @ lo,
           "two clusters": (q * np.where(np.arange(t) < t // 2, 1.0, 0.25)) @ q.conj().T,
           "16 decades": (q * 10.0 ** (-16.0 * np.arange(t) / (t - 1))) @ q.conj().T,
           "identity": np.eye(t, dtype=complex), "zero": np.zeros((t, t), dtype=complex)}
    for name, g in out.items():
        g = (g + g.conj().T) / 2
        top = np.linalg.eigvalsh(g).max()
        out[name] = g / top if top > 0 else g
    return out


def NUC_UNCERTAINTY(g, theta):
    """How far sum sqrt(lam) h(lam) can move when the eigenvalues move by t eps lam_max: the reference's own error (see the docstring)."""
    lam = np.linalg.eigvalsh(g)
    e = g.shape[0] * np.finfo(np.float64).eps * max(lam.max(), 0.0)

    def nuc(x):
        return np.maximum(np.sqrt(np.maximum(x, 0.0)) - theta, 0.0).sum()
    return float(nuc(lam + e) - nuc(lam - e))


def weight_call(k, grams, theta, with_step):
    b, t = grams.shape[0], grams.shape[1]
    gi = k.raw(torch.from_numpy(np.ascontiguousarray(R.to_pairs(grams))))
    if with_step:                                              # theta = step * thresh, both float32
        si, ti = k.raw(torch.tensor([0.5])), k.raw(torch.tensor([2.0 * theta]))
    else:
        si, ti = None, k.raw(torch.tensor([theta]))
    wo, info = k.out((b, t, t, 2)), k.out((b, 8))
    check(L().cine_svt_weight(ptr(gi), ptr(ti), ptr(si), wo.ptr(), info.ptr(), b, t, stream()), "cine_svt_weight")
    return [wo.t, info.t]


@pytest.mark.parametrize("frac", [0.0, 0.3, 1.5], ids=lambda f: f"th{f}")
@pytest.mark.parametrize("t", FRAMES, ids=lambda t: f"t{t}")
def test_weight_by_its_action(dev, t, frac):
    mats = gram_matrices(t)
    grams = np.stack(list(mats.values()))
    theta = float(np.float32(frac))                            # sigma_max = 1 for every matrix but the zero one
    w, info = twice(dev, 0, lambda k: weight_call(k, grams, theta, with_step=(t == 15)), f"cine_svt_weight t {t} threshold {frac}")
    w, info = R.to_complex(w), f64(info).reshape(len(mats), 4)
    for i, (name, g) in enumerate(mats.items()):
        what = f"cine_svt_weight t {t} {name} threshold {frac} sigma_max"
        w_ref, smax, nuc = LS.gram_weight(g, theta)
        assert np.array_equal(w[i], w[i].conj().T) and not np.diag(w[i]).imag.any(), what + ": W is not Hermitian"
        assert np.isfinite(info[i]).all(), (what, info[i])
        got_smax, got_nuc, resid, sweeps = info[i]
        if name == "zero" or frac > 1.0:
            assert not w[i].any() and got_nuc == 0.0, what + ": W is not exactly zero"
            act = 0.0
        else:
            act = float(np.abs(LS.gram_sqrt(g) @ (w[i] - w_ref)).max() / smax)
        slack = NUC_UNCERTAINTY(g, theta)
        print(f"{what}: action {act:.2e} (bar {BAR:.0e}); sigma_max {abs(got_smax - smax):.2e}, nuclear norm {abs(got_nuc - nuc):.2e} of {nuc:.3g} "
              f"(reference uncertain by {slack:.1e}); residual {resid:.1e}, {int(sweeps)} sweeps")
        assert act <= BAR, what
        assert abs(got_smax - smax) <= 1e-10 * smax and abs(got_nuc - nuc) <= 1e-10 * nuc + slack, what
        assert name in ("rank 3", "16 decades") and frac == 0.0 or slack <= 1e-12 * max(nuc, 1.0), (what, slack)
        assert resid <= 1e-14 and 0 <= sweeps < MAX_SWEEPS and sweeps == int(sweeps), what
        if name in ("identity", "zero"):
            assert sweeps == 0 and resid == 0.0, what


def test_a_nan_matrix_ends_at_the_cap_with_a_nan_residual(dev):
    g = np.stack([np.full((5, 5), np.nan + 0j), gram_matrices(5)["full rank"]])
    gram = torch.from_numpy(np.ascontiguousarray(R.to_pairs(g))).to(dev)
    th = torch.tensor([0.3], device=dev)
    w = torch.zeros((2, 5, 5, 2), device=dev)
    info = torch.zeros((2, 4), device=dev, dtype=torch.float64)
    check(L().cine_svt_weight(gram.data_ptr(), th.data_ptr(), None, w.data_ptr(), info.data_ptr(), 2, 5, stream()), "cine_svt_weight")
    torch.cuda.synchronize()
    info = info.cpu().numpy()
    assert np.isnan(info[0, 2]) and info[0, 3] == MAX_SWEEPS and info[1, 2] <= 1e-14 and bool(torch.isfinite(w[1]).all())


# ------------------------------------------------------------------ the prox
def prox_operands(shape, seed):
    b, t, h, w = shape
    return rnd(seed, b, t, h, w, 2), rnd(seed + 1, b, t, h, w, 2), rnd(seed + 2, b, t, h, w, 2)


def host_weight(l, g, theta):
    """W of the float32 v = l - step g in float64 (numpy.linalg.eigh), as the complex64 pairs the kernel is handed."""
    v = R.to_complex(l) - float(np.float32(STEP)) * R.to_complex(g)
    w = np.stack([LS.gram_weight(m, theta)[0] for m in LS.gram(v)])
    return torch.from_numpy(R.to_pairs(w).astype(np.float32)), v


def prox_call(k, l, s, g, wgt, thresh_s, shape, inplace=False, record=True):
    b, t, h, w = shape
    gi, wi, si, ti = k.inp(g), k.inp(wgt), k.raw(torch.tensor([STEP])), k.raw(torch.tensor([thresh_s]))
    if inplace:
        lo, so = k.out((b, t, h, w, 2), fill=l), k.out((b, t, h, w, 2), fill=s)
        li, s_in = lo.t, so.t
    else:
        li, s_in = k.inp(l), k.inp(s)
        lo, so = k.out((b, t, h, w, 2)), k.out((b, t, h, w, 2))
    xo = k.out((b, t, h, w, 2))
    rec = k.out((4,)) if record else None
    nbytes = L().cine_ls_prox_ws_bytes(b, t, h, w) if record else 0
    assert not record or nbytes == -(-h * w // 64) * b * 16
    ws = k.ws(nbytes)
    check(L().cine_ls_prox(ptr(li), ptr(s_in), ptr(gi), ptr(wi), ptr(si), ptr(ti), lo.ptr(), so.ptr(), xo.ptr(), rec.ptr() if record else None,
                           b, t, h, w, ws.ptr() if ws else None, nbytes, stream()), "cine_ls_prox")
    return [lo.t, so.t, xo.t] + ([rec.t] if record else [])


def peak_err(got, want):
    peak = np.abs(want).max()
    return float(np.abs(R.to_complex(got) - want).max() / peak) if peak > 0 else float(np.abs(R.to_complex(got)).max())


def check_prox(dev, shape, seed):
    l, s, g = prox_operands(shape, seed)
    l64, s64, g64 = R.to_complex(l), R.to_complex(s), R.to_complex(g)
    step = float(np.float32(STEP))
    for kind in ("zero", "mid"):
        v_l, v_s = l64 - step * g64, s64 - step * g64
        if kind == "zero":
            th_l = th_s = 0.0
        else:
            th_l = 0.3 * LS.sigma_max(v_l) / step
            th_s = float(np.float32(np.median(np.abs(R.fft1c(v_s, 1))) / step))
        wgt, _ = host_weight(l, g, step * th_l)
        what = f"cine_ls_prox {shape} thresholds {kind}"
        lnew, snew, xsum, rec = twice(dev, 2, lambda k: prox_call(k, l, s, g, wgt, th_s, shape), what)
        want_l, want_s, want_rec = LS.prox(l64, s64, g64, step, th_l, th_s)
        if kind == "zero":
            assert np.allclose(want_l, v_l, rtol=0, atol=1e-12) and np.allclose(want_s, v_s, rtol=0, atol=1e-12)      # the yardstick itself
        el, es, ex = peak_err(lnew, want_l), peak_err(snew, want_s), peak_err(xsum, want_l + want_s)
        er = [abs(float(rec[q]) - want_rec[q]) / want_rec[q] for q in range(3)]
        print(f"{what}: lnew {el:.2e}, snew {es:.2e}, xsum {ex:.2e} of the float64 peak (bar {BAR:.0e}); sums {er[0]:.2e} {er[1]:.2e} {er[2]:.2e} "
              f"relative (bar {SUM_REL:.0e})")
        assert max(el, es, ex) <= BAR, what
        assert max(er) <= SUM_REL and float(rec[3]) == 0.0, (what, er)
        k = Call(dev, 2)
        li, si, xi, ri = prox_call(k, l, s, g, wgt, th_s, shape, inplace=True)
        k.finish(what + " in place")
        assert same_bits(li.cpu(), lnew) and same_bits(si.cpu(), snew) and same_bits(xi.cpu(), xsum) and same_bits(ri.cpu(), rec), \
            what + ": in place gives other bits"
        k = Call(dev, 0)
        ln, sn, xn = prox_call(k, l, s, g, wgt, th_s, shape, record=False)
        k.finish(what + " without a record")
        assert same_bits(ln.cpu(), lnew) and same_bits(sn.cpu(), snew) and same_bits(xn.cpu(), xsum), what + ": other bits without the record"


@pytest.mark.parametrize("kind", KINDS, ids=lambda p: f"pix{p}")
@pytest.mark.parametrize("t", FRAMES, ids=lambda t: f"t{t}")
def test_prox_vs_float64(dev, t, kind):
    n = pixels(kind, 64)
    check_prox(dev, (1, t, 7, 9) if n == 63 else (1, t, 8, 8) if n == 64 else (1, t, 5, 13) if n == 65 else (1, t, n, 1), seed=2000 * t + n)


def test_prox_vs_float64_batch_two(dev):
    check_prox(dev, (2, 5, 5, 13), seed=77)


def test_the_three_kernels_chained_on_the_device_and_the_binding(dev):
    """gram -> weight -> prox as the solve chains them, against the yardstick's SVD; the binding gives the bits of the C calls."""
    from cine_hip import ops
    shape = (2, 15, 9, 17)
    l, s, g = prox_operands(shape, 5)
    step = float(np.float32(STEP))
    v_l = R.to_complex(l) - step * R.to_complex(g)
    th_l = float(np.float32(0.3 * LS.sigma_max(v_l) / step))
    th_s = float(np.float32(np.median(np.abs(R.fft1c(R.to_complex(s) - step * R.to_complex(g), 1))) / step))
    ld, sd, gd = l.to(dev), s.to(dev), g.to(dev)
    st, tl, ts = (torch.tensor([v], device=dev) for v in (STEP, th_l, th_s))
    gram = ops.casorati_gram(ld, gd, st)
    wgt, info = ops.svt_weight(gram, tl, st)
    lnew, snew, xsum, rec = ops.ls_prox(ld, sd, gd, wgt, st, ts, record=True)
    want_l, want_s, want_rec = LS.prox(R.to_complex(l), R.to_complex(s), R.to_complex(g), step, th_l, th_s)
    assert peak_err(lnew.cpu(), want_l) <= BAR and peak_err(snew.cpu(), want_s) <= BAR and peak_err(xsum.cpu(), want_l + want_s) <= BAR
    assert abs(float(info[:, 1].sum()) - want_rec[3]) <= 1e-6 * want_rec[3]             # v is rounded to float32 before the Gram matrix
    assert float(info[:, 2].max()) <= 1e-14
    (g_c,) = twice(dev, 0, lambda k: gram_call(k, l, g, shape), "cine_casorati_gram")
    assert torch.equal(g_c.view(torch.float64).reshape(gram.shape), gram.cpu())
    c = twice(dev, 0, lambda k: prox_call(k, l, s, g, wgt.cpu(), th_s, shape), "cine_ls_prox")
    assert all(same_bits(a, b.cpu()) for a, b in zip(c, (lnew, snew, xsum, rec)))
    l2, s2 = ld.clone(), sd.clone()
    a, b, x2 = ops.ls_prox(l2, s2, gd, wgt, st, ts, lnew=l2, snew=s2)                   # in place through the binding
    assert a.data_ptr() == l2.data_ptr() and b.data_ptr() == s2.data_ptr()
    assert same_bits(l2, lnew) and same_bits(s2, snew) and same_bits(x2, xsum)


# ------------------------------------------------------------------ refusals
def test_gram_refusals_come_before_anything_is_written(dev):
    shape = (1, 5, 5, 13)
    b, t, h, w = shape
    a, g, _ = prox_operands(shape, 3)
    k = Call(dev, 0)
    ai, gi, si = k.inp(a), k.inp(g), k.raw(torch.tensor([STEP]))
    out = k.out((b, t, t, 4))
    need = L().cine_casorati_gram_ws_bytes(b, t, h, w)
    ws = k.ws(need)
    base = dict(a=ptr(ai), g=ptr(gi), step=ptr(si), gram=out.ptr(), b=b, t=t, h=h, w=w, ws=ws.ptr(), nbytes=need)

    def call(**kw):
        c = {**base, **kw}
        return lambda: L().cine_casorati_gram(c["a"], c["g"], c["step"], c["gram"], c["b"], c["t"], c["h"], c["w"], c["ws"], c["nbytes"], stream())
    refused(call(t=1), EUNSUPPORTED, k, "cine_casorati_gram t = 1")
    refused(call(t=65), EUNSUPPORTED, k, "cine_casorati_gram t = 65")
    refused(call(b=65536), EUNSUPPORTED, k, "cine_casorati_gram b = 65536")
    for n in ("a", "gram", "ws", "step"):
        refused(call(**{n: None}), EINVAL, k, f"cine_casorati_gram {n} = NULL")
    for n in ("b", "t", "h", "w"):
        refused(call(**{n: 0}), EINVAL, k, f"cine_casorati_gram {n} = 0")
    refused(call(gram=base["a"]), EINVAL, k, "cine_casorati_gram gram aliases a")
    refused(call(gram=base["ws"]), EINVAL, k, "cine_casorati_gram gram aliases ws")
    refused(call(gram=base["gram"] + 8), EINVAL, k, "cine_casorati_gram gram off a 16-byte boundary")
    refused(call(nbytes=need - 1), EWORKSPACE, k, "cine_casorati_gram a workspace one byte short")
    check(call()(), "cine_casorati_gram")
    k.finish("cine_casorati_gram")
    assert bool(torch.isfinite(out.t).all())


def test_weight_refusals_come_before_anything_is_written(dev):
    g = np.stack([gram_matrices(5)["full rank"]])
    k = Call(dev, 0)
    gi = k.raw(torch.from_numpy(np.ascontiguousarray(R.to_pairs(g))))
    ti, si = k.raw(torch.tensor([0.3])), k.raw(torch.tensor([1.0]))
    wo, info = k.out((1, 5, 5, 2)), k.out((1, 8))
    base = dict(gram=ptr(gi), thresh=ptr(ti), step=ptr(si), weight=wo.ptr(), info=info.ptr(), b=1, t=5)

    def call(**kw):
        c = {**base, **kw}
        return lambda: L().cine_svt_weight(c["gram"], c["thresh"], c["step"], c["weight"], c["info"], c["b"], c["t"], stream())
    refused(call(t=1), EUNSUPPORTED, k, "cine_svt_weight t = 1")
    refused(call(t=65), EUNSUPPORTED, k, "cine_svt_weight t = 65")
    refused(call(b=65536), EUNSUPPORTED, k, "cine_svt_weight b = 65536")
    for n in ("gram", "thresh", "weight", "info"):
        refused(call(**{n: None}), EINVAL, k, f"cine_svt_weight {n} = NULL")
    for n in ("b", "t"):
        refused(call(**{n: 0}), EINVAL, k, f"cine_svt_weight {n} = 0")
    refused(call(weight=base["gram"]), EINVAL, k, "cine_svt_weight weight aliases gram")
    refused(call(info=base["weight"]), EINVAL, k, "cine_svt_weight info aliases weight")
    check(call()(), "cine_svt_weight")
    check(call(step=None)(), "cine_svt_weight")
    k.finish("cine_svt_weight")
    assert bool(torch.isfinite(wo.t).all()) and bool(torch.isfinite(info.t.view(torch.float64)).all())


def test_prox_refusals_come_before_anything_is_written(dev):
    shape = (1, 5, 5, 13)
    b, t, h, w = shape
    l, s, g = prox_operands(shape, 3)
    wgt, _ = host_weight(l, g, 0.5)
    k = Call(dev, 0)
    li, s_in, gi, wi = k.inp(l), k.inp(s), k.inp(g), k.inp(wgt)
    si, ti = k.raw(torch.tensor([STEP])), k.raw(torch.tensor([0.5]))
    lo, so, xo, rec = k.out((b, t, h, w, 2)), k.out((b, t, h, w, 2)), k.out((b, t, h, w, 2)), k.out((4,))
    need = L().cine_ls_prox_ws_bytes(b, t, h, w)
    ws = k.ws(need)
    base = dict(l=ptr(li), s=ptr(s_in), g=ptr(gi), weight=ptr(wi), step=ptr(si), thresh=ptr(ti), lnew=lo.ptr(), snew=so.ptr(), xsum=xo.ptr(),
                rec=rec.ptr(), b=b, t=t, h=h, w=w, ws=ws.ptr(), nbytes=need)

    def call(**kw):
        c = {**base, **kw}
        return lambda: L().cine_ls_prox(c["l"], c["s"], c["g"], c["weight"], c["step"], c["thresh"], c["lnew"], c["snew"], c["xsum"], c["rec"],
                                        c["b"], c["t"], c["h"], c["w"], c["ws"], c["nbytes"], stream())
    refused(call(t=1), EUNSUPPORTED, k, "cine_ls_prox t = 1")
    refused(call(t=65), EUNSUPPORTED, k, "cine_ls_prox t = 65")
    refused(call(b=65536), EUNSUPPORTED, k, "cine_ls_prox b = 65536")
    for n in ("l", "s", "g", "weight", "step", "thresh", "lnew", "snew", "xsum", "ws"):
        refused(call(**{n: None}), EINVAL, k, f"cine_ls_prox {n} = NULL")
    for n in ("b", "t", "h", "w"):
        refused(call(**{n: 0}), EINVAL, k, f"cine_ls_prox {n} = 0")
    refused(call(lnew=base["snew"]), EINVAL, k, "cine_ls_prox lnew aliases snew")
    refused(call(lnew=base["s"]), EINVAL, k, "cine_ls_prox lnew aliases s")
    refused(call(snew=base["l"]), EINVAL, k, "cine_ls_prox snew aliases l")
    refused(call(lnew=base["g"]), EINVAL, k, "cine_ls_prox lnew aliases g")
    refused(call(xsum=base["l"]), EINVAL, k, "cine_ls_prox xsum aliases l")
    refused(call(xsum=base["lnew"]), EINVAL, k, "cine_ls_prox xsum aliases lnew")
    refused(call(snew=base["weight"]), EINVAL, k, "cine_ls_prox snew aliases weight")
    refused(call(rec=base["xsum"]), EINVAL, k, "cine_ls_prox rec aliases xsum")
    refused(call(rec=base["ws"]), EINVAL, k, "cine_ls_prox rec aliases ws")
    refused(call(nbytes=need - 1), EWORKSPACE, k, "cine_ls_prox a workspace one byte short")
    check(call()(), "cine_ls_prox")
    k.finish("cine_ls_prox")
    assert bool(torch.isfinite(xo.t).all()) and bool(torch.isfinite(rec.t).all())
