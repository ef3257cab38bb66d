"""The pack, rotation and XPD buffer entry points of include/cine_hip.h and their adjoints (csrc/pack_kernels.hip, xpd_kernels.hip,
train_kernels.hip) called one by one through the C ABI, shape by shape, against float64 references on the CPU.

Entry points
  N  2-D halves: cine_normunet_pack (norm 1 / 0), cine_normunet_unpack (stats / NULL), cine_normunet_pack_bwd, cine_normunet_unpack_bwd
  V  3-D halves: cine_normunet3d_pack (norm 1 / 0: two kernels), cine_normunet3d_unpack
  R  rotations: cine_xfyf_pack, cine_xfyf_unpack, cine_xfyf_pack_bwd, cine_xfyf_unpack_bwd (xf 0 / 1, norm on / off) and the size functions
  X  XPD buffers: cine_xpd_pack, cine_xpd_unpack, cine_xpd_pack_bwd, cine_xpd_unpack_bwd, cine_xpd_ws_bytes, cine_chanlast_to_planes,
     cine_planes_to_chanlast, cine_extract_complex, cine_repeat_complex
  E  element-wise: cine_complex_abs, cine_complex_abs_bwd, cine_rss_normalise_bwd
  host only (no GPU): cine_pad16, cine_mwcnn_pad

References: every operation restated in float64 torch below (repack, group norm with the unbiased std, the floor / ceil pad split, the
temporal mean, fft1c and XPDNet's own ifftshift(fft(fftshift(.))), the 0.5 (xf + yf) average, the channel n that is appended and
dropped); inputs are the float32 values the kernel sees, widened.  The adjoint references are float64 autograd of the same restatements.
Unmarked CPU tests hold the restatements to 1e-10 against the oracle (NormUnet, NormUnet3D, VarNetBlock / XPDNetBlock.xfyf_transform with
a fixed linear module in place of the network, pad_for_mwcnn, complex_ops).

The bar: max |d| / peak of the reference against kernel_sweep.BAR.  The group norm cancels, so inputs come as "rand" (zero mean, unit
scale) and, on planes of at least 255 elements, "offset" (mean = 30 x std); a CPU test holds torch's own float32 result on every
(shape, family) of the lists to BAR / 2, which is what lets the GPU tests use the fixed bar.  Statistics are an output in their own right:
the means against the peak mean, the stds against the peak std.  The dstats of the unpack adjoints are dot products and are measured
against their cancellation-free scale sum |g q| (as cine_dot is in test_cg_kernels.py).  The gradient of the group norm is degenerate on
tiny planes: two values normalise to +-1/sqrt(2) whatever they are, the exact gradient of the planes' term is 0 and what is left is the
rounding of terms of size |gp| / std.  Wherever a normalised plane has fewer than 16 elements the pack adjoints are therefore judged
against max |gp| / std + |dmean| / N + |dstd| max |p| / (N - 1) (norm_bwd_scale) where that exceeds the reference's peak.

Every GPU case checks: the error; every float pointer at storage offsets of 0 and 2 floats (complex operands ask for 8-byte alignment)
with the same bits at both; a second call gives the same bits; a NaN prefill of every output between intact guard floats, pad frames
exactly 0; inputs bit-unchanged; workspaces of exactly the size *_ws_bytes returns, prefilled with NaN patterns, sentinel tail intact.
For the linear maps <A x, y> = <x, A^H y> is evaluated in float64 on the device's own outputs at BAR of the cancellation-free scale.
Refusals are decided on the host before any launch.  DESIGN.md section 4e has the measured worst error / bar per entry point, the
float32 yardsticks and the mutations the sweep was tried against.
"""
import ctypes
import functools

import pytest
import torch
import torch.nn.functional as F

from kernel_sweep import (BAR, EINVAL, EUNSUPPORTED, EWORKSPACE, Call, L, Worst, at_offsets, cap_samples, case_id, check, hash_case,
                          refused, same_bits, stream, twice)
from test_transform_kernels import _rand

PIN = 1e-10                                    # float64 restatement against the float64 oracle
OFFS = (0, 2)                                  # storage offsets in floats: complex operands must be 8-byte aligned (cine_hip.h)
# the constants of the kernels, restated: the reach test recomputes the paths from them
K_PACK_REGS, K_PIX, K_XPIX, K_XROWS, LDS_LIMIT = 16, 64, 32, 25, 64 * 1024
TINY = 16                                      # planes under 16 elements: the pack adjoint is judged against norm_bwd_scale
OFFSET_MIN = 255                               # "offset" inputs only on planes of at least 255 elements


# ================================================================== float64 references (CPU; they also run in float32 as the yardstick)
def pad16(n):
    return ((n - 1) | 15) + 1


def split16(n, norm=True):
    """Padded size and the left pad: floor on the left, ceil on the right (norm_unet.py:82-83); no padding without the norm."""
    m = pad16(n) if norm else n
    return m, (m - n) // 2


def mw_pad(size, n_scales):
    """utils/padding.py:26-47 for one dimension: padded size, left, right; odd sizes get the extra element on the left."""
    m = 1 << n_scales
    n_pad = 0 if size % m == 0 else (size // m + 1) * m - size
    left = n_pad // 2 if (size % 2 == 0 or n_pad == 0) else 1 + n_pad // 2
    return size + left + n_pad // 2, left, n_pad // 2


def ref_pack(x, norm):
    """x (n, *dims, 2) -> planes (n, 2, *padded dims), stats (n, 2, {mean, std}) or None: complex_to_chan_dim, group norm over each
    (sample, re | im) with the unbiased std, zero pad to multiples of 16 (norm_unet.py:48-86, 149-189)."""
    n, dims = x.shape[0], tuple(x.shape[1:-1])
    p = x.movedim(-1, 1)
    if not norm:
        return p.contiguous(), None
    g = p.reshape(n, 2, -1)
    mean, std = g.mean(dim=2), g.std(dim=2)
    sh = (n, 2) + (1,) * len(dims)
    p = (p - mean.view(sh)) / std.view(sh)
    pad = []
    for d in reversed(dims):
        m, lo = split16(d)
        pad += [lo, m - d - lo]
    return F.pad(p, pad), torch.stack([mean, std], dim=2)


def ref_unpack(planes, stats, dims):
    """The way back: crop the pad frame, x * std + mean, channels to the trailing pair (norm_unet.py:88-96, 71-74, 53-57)."""
    p = planes
    if stats is not None:
        sl = [slice(None), slice(None)]
        for d in dims:
            m, lo = split16(d)
            sl.append(slice(lo, lo + d))
        sh = (p.shape[0], 2) + (1,) * len(dims)
        p = p[tuple(sl)] * stats[:, :, 1].view(sh) + stats[:, :, 0].view(sh)
    return p.movedim(1, -1).contiguous()


def fft1c_t(z, dim, inverse=False):
    """fftc.py:5-56 on a complex tensor: fftshift(fft(ifftshift(.))), ortho."""
    f = torch.fft.ifft if inverse else torch.fft.fft
    return torch.fft.fftshift(f(torch.fft.ifftshift(z, dim=dim), dim=dim, norm="ortho"), dim=dim)


def xpd_fft_t(z, dim):
    """xpdnet.py:466: ifftshift(fft(fftshift(.))), the other shift order -- differs from fft1c for odd lengths.  Its inverse (:500) is
    fftshift(ifft(ifftshift(.))) = ifft1c."""
    return torch.fft.ifftshift(torch.fft.fft(torch.fft.fftshift(z, dim=dim), dim=dim, norm="ortho"), dim=dim)


def ref_xfyf_pack(img, xf, norm):
    """varnet.py:202-217 + both NormUnet front halves.  img (b, t, h, w, 2) -> planes_xf (b h, 2, W, T), planes_yf (b w, 2, H, T), stats_xf,
    stats_yf, mean_img (b, h, w, 2)."""
    b, t, h, w, _ = img.shape
    z = torch.view_as_complex(img.contiguous())
    mean = z.mean(dim=1)
    x = z - mean[:, None]
    if xf:
        x = fft1c_t(x, 1)
    xfz = torch.view_as_real(x.permute(0, 2, 3, 1).reshape(b * h, w, t).contiguous())
    yfz = torch.view_as_real(x.permute(0, 3, 2, 1).reshape(b * w, h, t).contiguous())
    pxf, sxf = ref_pack(xfz, norm)
    pyf, syf = ref_pack(yfz, norm)
    return pxf, pyf, sxf, syf, torch.view_as_real(mean)


def ref_xfyf_unpack(pxf, pyf, sxf, syf, mean, shape, xf):
    """varnet.py:229-241: both back halves, un-rotate, 0.5 (xf + yf), ifft1c over t, + the temporal mean.  out (b, t, h, w, 2)."""
    b, t, h, w = shape
    xz = torch.view_as_complex(ref_unpack(pxf, sxf, (w, t))).view(b, h, w, t)
    yz = torch.view_as_complex(ref_unpack(pyf, syf, (h, t))).view(b, w, h, t).permute(0, 2, 1, 3)
    out = 0.5 * (xz + yz)
    if xf:
        out = fft1c_t(out, 3, inverse=True)
    return torch.view_as_real(out.permute(0, 3, 1, 2) + torch.view_as_complex(mean.contiguous())[:, None])


def _mw(x, n_scales):
    (_, lt, rt), (_, li, ri) = mw_pad(x.shape[-1], n_scales), mw_pad(x.shape[-2], n_scales)
    return F.pad(x, [lt, rt, li, ri])


def ref_xpd_pack(buf, extra, n, n_scales, xf):
    """xpdnet.py:424-471.  buf (b, t, h, w, 2n) [re_0.., im_0..], extra (b, t, h, w, 2) appended as complex channel n -> planes_xf
    (b h, 2(n+1), pad(w), pad(t)), planes_yf (b w, 2(n+1), pad(h), pad(t)), mean (b, h, w, n+1, 2)."""
    b, t, h, w, _ = buf.shape
    z = torch.cat([torch.complex(buf[..., :n], buf[..., n:]), torch.view_as_complex(extra.contiguous())[..., None]], dim=-1)
    mean = z.mean(dim=1)
    x = z - mean[:, None]
    if xf:
        x = xpd_fft_t(x, 1)
    r = torch.cat([x.real, x.imag], dim=-1)                                        # (b, t, h, w, 2 (n + 1))
    pxf = r.permute(0, 2, 4, 3, 1).reshape(b * h, 2 * (n + 1), w, t)
    pyf = r.permute(0, 3, 4, 2, 1).reshape(b * w, 2 * (n + 1), h, t)
    return _mw(pxf, n_scales), _mw(pyf, n_scales), torch.view_as_real(mean)


def ref_xpd_unpack(pxf, pyf, mean, shape, n, n_scales, xf):
    """xpdnet.py:485-509: unpad, un-rotate, average, fftshift(ifft(ifftshift(.))), + the temporal mean of channels 0 .. n-1 (channel n is
    dropped).  planes carry 2n channels; out (b, t, h, w, 2n)."""
    b, t, h, w = shape
    (_, lt, _), (_, lw, _), (_, lh, _) = mw_pad(t, n_scales), mw_pad(w, n_scales), mw_pad(h, n_scales)
    x = pxf[:, :, lw:lw + w, lt:lt + t].reshape(b, h, 2 * n, w, t).permute(0, 4, 1, 3, 2)
    y = pyf[:, :, lh:lh + h, lt:lt + t].reshape(b, w, 2 * n, h, t).permute(0, 4, 3, 1, 2)
    out = 0.5 * (x + y)
    if xf:
        z = fft1c_t(torch.complex(out[..., :n], out[..., n:]), 1, inverse=True)
        out = torch.cat([z.real, z.imag], dim=-1)
    m = torch.view_as_complex(mean.contiguous())[..., :n]
    return out + torch.cat([m.real, m.imag], dim=-1)[:, None]


def ref_chanlast_to_planes(x, n_scales):
    return _mw(x.permute(0, 3, 1, 2), n_scales).contiguous()


def ref_planes_to_chanlast(p, h, w, n_scales):
    (_, lh, _), (_, lw, _) = mw_pad(h, n_scales), mw_pad(w, n_scales)
    return p[:, :, lh:lh + h, lw:lw + w].permute(0, 2, 3, 1).contiguous()


def ref_rss_normalise(x):
    """varnet.py:58-59: x (b, c, h, w, 2) / rss over the coil axis."""
    return x / x.pow(2).sum(dim=(1, 4), keepdim=True).sqrt()


def vjp(fn, ins, gouts):
    """Float64 autograd: the gradients of sum_k <fn(ins)[k], gouts[k]> with respect to every input."""
    with torch.enable_grad():
        ins = [i.detach().clone().requires_grad_(True) for i in ins]
        outs = fn(*ins)
        outs = outs if isinstance(outs, (tuple, list)) else [outs]
        s = sum((o * g).sum() for o, g in zip(outs, gouts) if o is not None and g is not None)
        gr = torch.autograd.grad(s, ins, allow_unused=True)
    return [torch.zeros_like(i) if g is None else g for i, g in zip(ins, gr)]


def norm_bwd_scale(gp, p, stats, dstats, cnt):
    """The size of the terms cine_normunet_pack_bwd adds up: max |gp| / std + |dmean| / N + |dstd| max |p| / (N - 1), the largest over
    (sample, re | im)."""
    n = gp.shape[0]
    g, q = gp.reshape(n, 2, -1).abs().amax(dim=2), p.reshape(n, 2, -1).abs().amax(dim=2)
    return float((g / stats[:, :, 1] + dstats[:, :, 0].abs() / cnt + dstats[:, :, 1].abs() * q / (cnt - 1)).max())


# ================================================================== case lists
def pack_threads(cnt):
    for nt in (256, 512, 1024):
        if cnt <= K_PACK_REGS * nt:
            return nt
    return 1024


def pack_path(cnt, nt=None):
    """(threads, in registers) of normunet_pack_kernel for a plane of cnt elements launched with nt threads (its own choice by default)."""
    nt = nt or pack_threads(cnt)
    return nt, cnt <= K_PACK_REGS * nt


N_PLANES = [(1, 2), (2, 1), (15, 17), (16, 16), (64, 64), (17, 241), (64, 128), (3, 2731), (128, 128), (5, 3277), (200, 200)]
N_SAMPLES = [1, 2, 5]
V_VOLUMES = [(1, 1, 2), (2, 3, 5), (5, 9, 11), (16, 16, 16), (3, 17, 33), (15, 40, 36)]


def _families(cnt):
    return ["rand", "offset"] if cnt >= OFFSET_MIN else ["rand"]


N_CASES = [dict(h=h, w=w, n=cap_samples(N_SAMPLES[(i + j) % 3], h * w, 82_000 if h * w < 40_000 else 40_000), fam=fam)      # 200 x 200: one sample
           for i, (h, w) in enumerate(N_PLANES) for j, fam in enumerate(_families(h * w))]
V_CASES = [dict(t=t, h=h, w=w, n=1 + (i + j) % 2, fam=fam) for i, (t, h, w) in enumerate(V_VOLUMES) for j, fam in enumerate(_families(t * h * w))]

# (t, h, w, b): t in {2, 3, 15, 16, 17, 64}, h w mod 64 in {1, 63, 0}, w in {1, 63, 64, 65, 130}, and the two mixed launches
R_SHAPES = [(2, 1, 1, 1), (3, 1, 63, 2), (15, 3, 64, 1), (16, 5, 65, 1), (17, 2, 130, 1), (64, 5, 13, 2), (15, 9, 7, 1),
            (64, 257, 3, 1), (33, 130, 5, 1)]
R_CASES = [dict(t=t, h=h, w=w, b=b, xf=xf, norm=norm) for (t, h, w, b) in R_SHAPES for xf in (0, 1) for norm in (1, 0)]

# (t, h, w, b, n_primal, n_scales)
X_SHAPES = [(2, 1, 1, 1, 1, 0), (3, 1, 31, 2, 5, 1), (15, 24, 32, 1, 1, 0), (16, 25, 33, 1, 5, 0), (3, 26, 65, 1, 1, 0), (2, 50, 3, 1, 15, 0),
            (15, 51, 2, 1, 5, 0), (3, 31, 5, 1, 1, 3), (16, 51, 3, 2, 1, 3)]
# the largest tiles the guards accept, one tiny plane each: what the forward accepts, its adjoint does not
X_EDGE = {"pack": [(17, 2, 3, 1, 14, 1)], "unpack": [(16, 2, 3, 1, 15, 1), (17, 2, 3, 1, 15, 1)],
          "unpack_bwd": [(16, 2, 3, 1, 15, 1), (17, 2, 3, 1, 15, 1)], "pack_bwd": [(9, 2, 3, 1, 13, 1)]}


def x_cases(entry):
    return [dict(t=t, h=h, w=w, b=b, n=n, ns=ns, xf=xf) for (t, h, w, b, n, ns) in X_SHAPES + X_EDGE[entry] for xf in (0, 1)]


def xpd_lds(entry, t, n):
    """Bytes of dynamic LDS the guards of xpd_kernels.hip / train_kernels.hip compute."""
    cols = {"pack": n + 1, "unpack": n, "unpack_bwd": n, "pack_bwd": 2 * (n + 1)}[entry]
    return (t * K_XPIX * cols + t) * 8


CHANLAST_CASES = [dict(n=1, c=1, h=5, w=4, ns=0), dict(n=2, c=2, h=7, w=9, ns=3), dict(n=1, c=12, h=6, w=5, ns=3), dict(n=2, c=12, h=8, w=8, ns=0),
                  dict(n=1, c=2, h=51, w=3, ns=3)]
EXTRACT_CASES = [dict(npix=1, c=2, c_re=0, c_im=1), dict(npix=257, c=3, c_re=1, c_im=1), dict(npix=1000, c=4, c_re=3, c_im=0)]
REPEAT_CASES = [dict(npix=1, n=1), dict(npix=257, n=5), dict(npix=3000, n=1), dict(npix=256, n=5)]
E_N = [1, 255, 256, 257, 65_537]
RSS_CASES = [dict(b=1, c=1, h=1, w=1), dict(b=2, c=2, h=3, w=85), dict(b=1, c=15, h=16, w=16), dict(b=2, c=15, h=257, w=1), dict(b=1, c=2, h=7, w=43)]


# ================================================================== inputs and references per case (CPU; shared by the tests)
def _input(seed, fam, *shape):
    x = _rand(seed, *shape)
    return x + 30.0 if fam == "offset" else x


def _stats(seed, n):
    """Statistics for the back halves: any mean, a std well away from 0."""
    s = _rand(seed, n, 2, 2)
    s[:, :, 1] = s[:, :, 1].abs() + 0.5
    return s


def _key(c):
    return tuple(sorted(c.items()))


def _dims(c):
    return (c["t"], c["h"], c["w"]) if "t" in c else (c["h"], c["w"])


@functools.lru_cache(maxsize=None)
def _nv_ref(key):
    """N and V: the input, the float64 front half and torch's own float32 one."""
    c = dict(key)
    x = _input(hash_case(c), c["fam"], c["n"], *_dims(c), 2)
    p, s = ref_pack(x.double(), True)
    p32, s32 = ref_pack(x, True)
    return dict(x=x, p=p, s=s, p32=p32, s32=s32)


def nv_ref(c):
    return _nv_ref(_key(c))


@functools.lru_cache(maxsize=None)
def _r_ref(key):
    c = dict(key)
    img = _rand(hash_case(c), c["b"], c["t"], c["h"], c["w"], 2)
    return dict(img=img, out=ref_xfyf_pack(img.double(), c["xf"], c["norm"]), out32=ref_xfyf_pack(img, c["xf"], c["norm"]))


def r_ref(c):
    return _r_ref(_key(c))


def stat_errs(got, ref):
    """Statistics as an output: the means against the peak mean, the stds against the peak std."""
    return max(float((got.double()[..., k] - ref[..., k]).abs().max() / ref[..., k].abs().max().clamp_min(1e-30)) for k in (0, 1))


def peak_err(got, ref, scale=None):
    scale = float(ref.abs().max().clamp_min(1e-30)) if scale is None else scale
    return float((got.double() - ref).abs().max()) / scale


# ================================================================== CPU tests: the restatements against the oracle
class _Mix(torch.nn.Module):
    """A fixed linear map of planes in place of the network (the same on both sides of a pin): mixes the two channel halves, shifts along
    the last axis, and keeps `keep` of every half's channels (XPDNet's image net returns 2n of 2(n + 1) channels)."""

    def __init__(self, keep=None):
        super().__init__()
        self.keep = keep

    def forward(self, x):
        y = 1.3 * x.flip(1) + 0.5 * torch.roll(x, 1, -1) + 0.1
        if self.keep is not None:
            half = x.shape[1] // 2
            y = torch.cat([y[:, :self.keep], y[:, half:half + self.keep]], dim=1)
        return y


def _normunet_with(mid, dims):
    from oracle import regularisers as R
    net = (R.NormUnet if dims == 2 else R.NormUnet3D)(2, 1)
    net.unet = mid
    return net.double()


@pytest.mark.parametrize("h,w", [(1, 2), (15, 17), (16, 16), (24, 20), (33, 17)])
def test_reference_halves_are_the_oracles_normunet(h, w):
    from oracle import regularisers as R
    x = _rand(h * 100 + w, 3, h, w, 2).double() + 2.0
    p, s = ref_pack(x, True)
    po, mo, so = R.NormUnet.norm(x.permute(0, 3, 1, 2))
    assert float((s[:, :, 0] - mo.view(3, 2)).abs().max()) < PIN and float((s[:, :, 1] - so.view(3, 2)).abs().max()) < PIN
    (hm, hp), (wm, wp) = R._pad16(h), R._pad16(w)
    assert p.shape == (3, 2, hm, wm) and (split16(h), split16(w)) == ((hm, hp[0]), (wm, wp[0]))
    assert float((p - F.pad(po, wp + hp)).abs().max()) < PIN
    mid = _Mix()
    want = _normunet_with(mid, 2)(x[:, None])[:, 0]                       # NormUnet.forward takes (b, c, h, w, 2)
    assert float((ref_unpack(mid(p), s, (h, w)) - want).abs().max()) < PIN
    assert torch.equal(ref_unpack(ref_pack(x, False)[0], None, (h, w)), x)


@pytest.mark.parametrize("t,h,w", [(1, 1, 2), (2, 3, 5), (5, 9, 11), (16, 16, 16), (3, 17, 33)])
def test_reference_halves_are_the_oracles_normunet3d(t, h, w):
    x = _rand(t * 1000 + h * 10 + w, 2, t, h, w, 2).double() - 1.5
    p, s = ref_pack(x, True)
    assert p.shape == (2, 2, pad16(t), pad16(h), pad16(w))
    mid = _Mix()
    want = _normunet_with(mid, 3)(x[:, None])[:, 0]
    assert float((ref_unpack(mid(p), s, (t, h, w)) - want).abs().max()) < PIN


@pytest.mark.parametrize("t,h,w,b", [(2, 1, 1, 1), (3, 1, 7, 2), (15, 6, 5, 1), (16, 5, 9, 2), (17, 4, 3, 1)])
@pytest.mark.parametrize("xf", [0, 1])
def test_reference_rotation_is_the_oracles_xfyf_transform(t, h, w, b, xf):
    """Pack then unpack pinned as a pair, with a fixed linear map between them (identity too): VarNetBlock.xfyf_transform over NormUnets."""
    from oracle import varnet_ref as V
    img = _rand(t * 50 + h * 7 + w + xf, b, t, h, w, 2).double() + 0.7
    for mid in (torch.nn.Identity(), _Mix()):
        blk = V.VarNetBlock(_normunet_with(mid, 2), "XF" if xf else "XT", True)
        want = blk.xfyf_transform(img)[:, :, 0]
        pxf, pyf, sxf, syf, mean = ref_xfyf_pack(img, xf, True)
        got = ref_xfyf_unpack(mid(pxf), mid(pyf), sxf, syf, mean, (b, t, h, w), xf)
        assert float((got - want).abs().max()) < PIN
        # norm off (CineNet feeds a bare Unet): the same rotation without the halves' norm and pad
        blk = V.VarNetBlock(_Bare(mid), "XF" if xf else "XT", True)
        pxf, pyf, _, _, mean = ref_xfyf_pack(img, xf, False)
        got = ref_xfyf_unpack(mid(pxf), mid(pyf), None, None, mean, (b, t, h, w), xf)
        assert float((got - blk.xfyf_transform(img)[:, :, 0]).abs().max()) < PIN


class _Bare(torch.nn.Module):
    """(n, 1, I, J, 2) -> planes (n, 2, I, J) -> mid -> back: the plain repack around a bare network (cinenet.py:242-244)."""

    def __init__(self, mid):
        super().__init__()
        self.mid = mid

    def forward(self, x):
        return self.mid(x[:, 0].permute(0, 3, 1, 2)).permute(0, 2, 3, 1)[:, None].contiguous()


@pytest.mark.parametrize("t,h,w,b,n,ns", [(2, 1, 1, 1, 1, 0), (3, 2, 7, 2, 5, 1), (15, 6, 5, 1, 2, 3), (16, 5, 9, 1, 1, 2), (5, 3, 4, 2, 3, 3)])
@pytest.mark.parametrize("xf", [0, 1])
def test_reference_xpd_halves_are_the_oracles_xfyf_transform(t, h, w, b, n, ns, xf):
    from oracle import xpdnet_ref as X
    buf, extra = _rand(t + h + w + n, b, t, h, w, 2 * n).double() + 0.3, _rand(t + h + w + n + 1, b, t, h, w, 2).double()
    ib = torch.cat([buf[..., :n], extra[..., :1], buf[..., n:], extra[..., 1:]], dim=-1)                # [re_0 .. re_n, im_0 .. im_n]
    mid = _Mix(keep=n)
    blk = X.XPDNetBlock(None, [mid], ns, "XF" if xf else "XT", True, dict(i_buffer_mode=True, k_buffer_mode=True, i_buffer_size=n, k_buffer_size=n))
    want = blk.xfyf_transform(ib, 0)[:, :, 0]
    pxf, pyf, mean = ref_xpd_pack(buf, extra, n, ns, xf)
    got = ref_xpd_unpack(mid(pxf), mid(pyf), mean, (b, t, h, w), n, ns, xf)
    assert float((got - want).abs().max()) < PIN


def test_the_two_centred_transforms_differ_exactly_for_odd_lengths():
    from oracle import centered_fft as C
    for t in (2, 3, 15, 16, 17):
        z = torch.view_as_complex(_rand(t, 4, t, 2).double())
        a, bb = fft1c_t(z, 1), xpd_fft_t(z, 1)
        assert float((torch.view_as_real(a) - C.fft1c(torch.view_as_real(z))).abs().max()) < PIN
        assert float((bb - C.xpd_temporal_fft(z, 1)).abs().max()) < PIN
        assert float((fft1c_t(z, 1, inverse=True) - C.xpd_temporal_ifft(z, 1)).abs().max()) < PIN
        assert (float((a - bb).abs().max()) < PIN) == (t % 2 == 0)


def test_reference_pads_and_element_wise_operations_are_the_oracles():
    from oracle import complex_ops as O
    from oracle import xpdnet_ref as X
    for ns in range(5):
        x = _rand(ns, 2, 3, 7, 10).double()
        want, pads = X.pad_for_mwcnn(x, ns)
        assert torch.equal(_mw(x, ns), want) and pads == [*mw_pad(10, ns)[1:], *mw_pad(7, ns)[1:]]
    x = _rand(5, 2, 3, 4, 5, 2).double()
    assert float((ref_rss_normalise(x) - x / O.rss_complex(x, dim=1)[:, None, ..., None]).abs().max()) < PIN
    assert float((torch.view_as_complex(x).abs() - O.complex_abs(x)).abs().max()) < PIN
    z = torch.view_as_complex(_rand(6, 7, 3, 2).double())
    buf = O.complex_to_real_multi_ch(z)                                   # [re_0 .. re_2, im_0 .. im_2]
    assert torch.equal(torch.view_as_real(O.real_to_complex_multi_ch(buf, 3)[..., 1]), torch.stack([buf[..., 1], buf[..., 4]], dim=-1))
    y = torch.repeat_interleave(torch.view_as_real(z[:, 0]), 5, dim=-1)   # xpdnet.py:306-307
    assert torch.equal(y, ref_repeat(torch.view_as_real(z[:, 0]).contiguous(), 5))


def ref_repeat(img, n):
    """repeat_interleave(image, n, dim=-1) of (npix, 2): [re x n, im x n]."""
    return torch.cat([img[:, :1].expand(-1, n), img[:, 1:].expand(-1, n)], dim=1).contiguous()


# ------------------------------------------------------------------ host only: the padding tables (the library loads without a GPU)
def test_pad16_table():
    from oracle import regularisers as R
    lib = L()
    for n in range(1, 601):
        m, (lo, hi) = R._pad16(n)
        assert lib.cine_pad16(n) == m == pad16(n) and split16(n) == (m, lo) and lo + hi == m - n


def test_mwcnn_pad_table():
    from oracle import xpdnet_ref as X
    lib = L()
    left, right = ctypes.c_int(-1), ctypes.c_int(-1)
    for ns in range(5):
        for size in range(1, 601):
            total = lib.cine_mwcnn_pad(size, ns, ctypes.addressof(left), ctypes.addressof(right))
            padded, pads = X.pad_for_mwcnn(torch.zeros(1, size), ns)
            assert (left.value, right.value, total) == (pads[0], pads[1], padded.shape[-1]), (size, ns)
            assert mw_pad(size, ns) == (total, left.value, right.value)
            assert lib.cine_mwcnn_pad(size, ns, None, None) == total


# ------------------------------------------------------------------ the case lists reach every branch
def test_case_lists_reach_every_branch():
    # N: thread count x register / streaming path, both sides of every threshold, every sample count, both families
    paths = {(c["h"] * c["w"],) + pack_path(c["h"] * c["w"]) for c in N_CASES}
    for want in [(2, 256, True), (4096, 256, True), (4097, 512, True), (8192, 512, True), (8193, 1024, True), (16384, 1024, True),
                 (16385, 1024, False), (40000, 1024, False)]:
        assert want in paths, want
    assert {c["n"] for c in N_CASES} == {1, 2, 5} and [c["n"] for c in N_CASES if c["h"] == 200] == [1, 1]
    assert {(c["h"], c["w"]) for c in N_CASES} == set(N_PLANES)
    for h, w in N_PLANES:
        fams = {c["fam"] for c in N_CASES if (c["h"], c["w"]) == (h, w)}
        assert fams == ({"rand", "offset"} if h * w >= OFFSET_MIN else {"rand"})
    # threads that hold no element on the register path (the clamp), pad on both sides with an odd split, no pad
    for nt in (256, 512, 1024):
        assert any(pack_path(c["h"] * c["w"]) == (nt, True) and c["h"] * c["w"] < K_PACK_REGS * nt for c in N_CASES), nt
    assert any(c["h"] * c["w"] < 256 for c in N_CASES)                   # whole waves without an element
    assert any((pad16(c["h"]) - c["h"]) % 2 and (pad16(c["w"]) - c["w"]) % 2 for c in N_CASES) and any(c["h"] % 16 == 0 and c["w"] % 16 == 0 for c in N_CASES)
    # V
    assert {(c["t"], c["h"], c["w"]) for c in V_CASES} == set(V_VOLUMES) and {c["n"] for c in V_CASES} == {1, 2}
    assert any(c["t"] % 16 == 0 and c["h"] % 16 == 0 and c["w"] % 16 == 0 for c in V_CASES) and any(c["t"] * c["h"] * c["w"] > 1024 for c in V_CASES)
    # R: frames, pixel tiles of the temporal kernels, column tiles of the unpack, both plane sets' launch paths
    assert {c["t"] for c in R_CASES} >= {2, 3, 15, 16, 17, 64} and {c["b"] for c in R_CASES} == {1, 2}
    assert {c["h"] * c["w"] % K_PIX for c in R_CASES} >= {1, 63, 0} and {c["w"] for c in R_CASES} >= {1, 63, 64, 65, 130}
    assert any(-(-c["w"] // K_PIX) == 3 for c in R_CASES) and any(-(-c["h"] * c["w"] // K_PIX) > 1 for c in R_CASES)
    assert {(c["xf"], c["norm"]) for c in R_CASES} == {(0, 0), (0, 1), (1, 0), (1, 1)}
    mixed = set()
    for c in R_CASES:
        cx, cy = c["w"] * c["t"], c["h"] * c["t"]
        nt = max(pack_threads(cx), pack_threads(cy))
        if pack_threads(cx) != pack_threads(cy):
            mixed.add((pack_path(cx, nt), pack_path(cy, nt)))
    assert ((1024, True), (1024, False)) in mixed, mixed            # (64, 257, 3): 192 elements in registers under the streaming set's 1024
    assert ((512, True), (512, True)) in mixed, mixed               # (33, 130, 5): the y-f set takes 512
    # X: every axis value, pixel tiles, row blocks (ragged and full), the largest tiles the guards accept and the first they refuse
    for entry in X_EDGE:
        cs = x_cases(entry)
        assert {c["n"] for c in cs} >= {1, 5, 15} and {c["ns"] for c in cs} >= {0, 1, 3} and {c["t"] for c in cs} >= {2, 3, 15, 16}
        assert {c["w"] for c in cs} >= {1, 31, 32, 33, 65} and {c["h"] * c["w"] % K_XPIX for c in cs} >= {1, 31, 0}
        assert {c["xf"] for c in cs} == {0, 1} and {c["b"] for c in cs} == {1, 2}
        assert all(xpd_lds(entry, c["t"], c["n"]) <= LDS_LIMIT for c in cs)
    rows = {(c["ns"], mw_pad(d, c["ns"])[0]) for c in x_cases("pack") for d in (c["h"], c["w"])}
    assert rows >= {(0, 24), (0, 25), (0, 26), (0, 50), (0, 51), (3, 32), (3, 56)}
    assert {r % K_XROWS for _, r in rows} >= {0, 1, 24} and {-(-r // K_XROWS) for _, r in rows} >= {1, 2, 3}
    assert xpd_lds("pack", 17, 14) == 65_416 and xpd_lds("pack", 16, 15) > LDS_LIMIT and xpd_lds("pack", 18, 14) > LDS_LIMIT
    assert xpd_lds("pack_bwd", 9, 13) == 64_584 and xpd_lds("pack_bwd", 8, 15) > LDS_LIMIT and xpd_lds("pack_bwd", 10, 13) > LDS_LIMIT
    assert xpd_lds("unpack", 16, 15) <= xpd_lds("unpack", 17, 15) == 65_416 and xpd_lds("unpack", 18, 15) > LDS_LIMIT
    # training refuses t (n + 1) > 127 where inference accepts up to 254, and 255 with t <= 32 (the t twiddles share the tile's LDS)
    for t in range(2, 65):
        for n in range(1, 16):
            tn = t * (n + 1)
            assert (xpd_lds("pack", t, n) <= LDS_LIMIT) == (tn <= 254 or (tn == 255 and t <= 32)) and (xpd_lds("pack_bwd", t, n) <= LDS_LIMIT) == (tn <= 127)
    assert {c["c"] for c in CHANLAST_CASES} == {1, 2, 12} and {c["ns"] for c in CHANLAST_CASES} == {0, 3}
    assert {(c["h"] % 2, c["w"] % 2) for c in CHANLAST_CASES} == {(0, 0), (0, 1), (1, 0), (1, 1)}
    assert any(c["c_re"] == c["c_im"] for c in EXTRACT_CASES) and any(c["c_im"] < c["c_re"] for c in EXTRACT_CASES)
    assert {c["n"] for c in REPEAT_CASES} == {1, 5} and {c["c"] for c in RSS_CASES} == {1, 2, 15} and {c["b"] for c in RSS_CASES} == {1, 2}
    assert any(c["h"] * c["w"] % 256 for c in RSS_CASES) and any(c["h"] * c["w"] > 256 for c in RSS_CASES)


# ------------------------------------------------------------------ the float32 yardstick
YARD = Worst()


@pytest.mark.parametrize("c", N_CASES + V_CASES, ids=case_id)
def test_float32_yardstick_of_the_group_norm(c):
    """torch's own float32 front half against the float64 one, for every (shape, family): at most BAR / 2 (measured: 1.1e-7 for "rand",
    7e-7 for "offset"), the condition for holding the device to the plain BAR."""
    d = nv_ref(c)
    YARD.record("planes " + c["fam"], peak_err(d["p32"], d["p"]), BAR / 2, case_id(c))
    YARD.record("stats " + c["fam"], stat_errs(d["s32"], d["s"]), BAR / 2, case_id(c))


@pytest.mark.parametrize("c", [c for c in R_CASES if c["norm"]], ids=case_id)
def test_float32_yardstick_of_the_rotation(c):
    d = r_ref(c)
    for name, a, r in zip(("planes_xf", "planes_yf"), d["out32"][:2], d["out"][:2]):
        YARD.record("rotation " + name, peak_err(a, r), BAR / 2, case_id(c))
    for name, a, r in zip(("stats_xf", "stats_yf"), d["out32"][2:4], d["out"][2:4]):
        # the rotated planes have zero temporal mean: their group means are rounding residue, so only the stds are an output to measure
        YARD.record("rotation " + name, float((a.double()[..., 1] - r[..., 1]).abs().max() / r[..., 1].abs().max()), BAR / 2, case_id(c))


def test_float32_yardstick_report():
    """Prints the yardsticks of the two tests above (run with -s); they are recorded in DESIGN.md 4e."""
    if YARD:
        YARD.report()


# ================================================================== GPU tests
gpu = pytest.mark.gpu
WORST = Worst()
_record = WORST.record


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "-m gpu tests need an MI355X"
    yield torch.device("cuda:0")
    if WORST:
        WORST.report()


def zero_frame(got, wins, what):
    """Pad frames come back exactly 0, not NaN.  wins: (left pad, size) of the window inside each trailing axis."""
    k = len(wins)
    frame = torch.ones(got.shape[-k:], dtype=torch.bool)
    frame[tuple(slice(lo, lo + d) for lo, d in wins)] = False
    assert not bool(got[(slice(None),) * (got.dim() - k) + (frame,)].any()), f"{what}: a pad element is not 0"


def wins16(*dims):
    return [(split16(d)[1], d) for d in dims]


def wins_mw(n_scales, *dims):
    return [(mw_pad(d, n_scales)[1], d) for d in dims]


def _mean_std_record(name, got, ref, case, means=True):
    g, r = got.double(), ref
    if means:
        _record(name + " mean", float((g[..., 0] - r[..., 0]).abs().max() / r[..., 0].abs().max().clamp_min(1e-30)), BAR, case)
    _record(name + " std", float((g[..., 1] - r[..., 1]).abs().max() / r[..., 1].abs().max().clamp_min(1e-30)), BAR, case)


# ------------------------------------------------------------------ N and V: the halves
def _pack_entry(c):
    if "t" in c:
        return "cine_normunet3d_pack", lambda x, p, s, norm: L().cine_normunet3d_pack(x, p, s, c["n"], c["t"], c["h"], c["w"], norm, stream())
    return "cine_normunet_pack", lambda x, p, s, norm: L().cine_normunet_pack(x, p, s, c["n"], c["h"], c["w"], norm, stream())


def _unpack_entry(c):
    if "t" in c:
        return "cine_normunet3d_unpack", lambda p, s, y: L().cine_normunet3d_unpack(p, s, y, c["n"], c["t"], c["h"], c["w"], stream())
    return "cine_normunet_unpack", lambda p, s, y: L().cine_normunet_unpack(p, s, y, c["n"], c["h"], c["w"], stream())


@gpu
@pytest.mark.parametrize("c", N_CASES + V_CASES, ids=case_id)
def test_pack(dev, c):
    d = nv_ref(c)
    name, entry = _pack_entry(c)

    def body(k):
        x, p, s = k.inp(d["x"]), k.out(d["p"].shape), k.out(d["s"].shape)
        check(entry(x.data_ptr(), p.ptr(), s.ptr(), 1), name)
        return [p.t, s.t]
    p, s = at_offsets(dev, OFFS, body, name)
    _record(name, peak_err(p, d["p"]), BAR, case_id(c))
    _mean_std_record(name, s, d["s"], case_id(c))
    zero_frame(p, wins16(*_dims(c)), name)
    if c["fam"] == "rand":                                           # norm == 0: a pure repack, stats may be NULL
        ref = ref_pack(d["x"], False)[0]

        def plain(k):
            x, p = k.inp(d["x"]), k.out(ref.shape)
            check(entry(x.data_ptr(), p.ptr(), None, 0), name)
            return [p.t]
        p, = at_offsets(dev, OFFS, plain, name + " norm=0")
        assert same_bits(p, ref), f"{name} norm=0 is not a pure repack"


@gpu
@pytest.mark.parametrize("c", [c for c in N_CASES + V_CASES if c["fam"] == "rand"], ids=case_id)
def test_unpack(dev, c):
    name, entry = _unpack_entry(c)
    dims, n = _dims(c), c["n"]
    seed = hash_case(c)
    q, st = _rand(seed + 1, n, 2, *[pad16(v) for v in dims]), _stats(seed + 2, n)
    ref = ref_unpack(q.double(), st.double(), dims)

    def body(k):
        qd, sd, y = k.inp(q), k.inp(st), k.out(ref.shape)
        check(entry(qd.data_ptr(), sd.data_ptr(), y.ptr()), name)
        return [y.t]
    y, = at_offsets(dev, OFFS, body, name)
    _record(name, peak_err(y, ref), BAR, case_id(c))
    q0 = _rand(seed + 3, n, 2, *dims)

    def plain(k):
        qd, y = k.inp(q0), k.out(ref.shape)
        check(entry(qd.data_ptr(), None, y.ptr()), name)
        return [y.t]
    y, = at_offsets(dev, OFFS, plain, name + " stats=NULL")
    assert same_bits(y, ref_unpack(q0, None, dims)), f"{name} with NULL stats is not a pure gather"


N_RAND = [c for c in N_CASES if c["fam"] == "rand"]


@gpu
@pytest.mark.parametrize("c", N_RAND, ids=case_id)
def test_normunet_unpack_bwd(dev, c):
    name, (h, w), n = "cine_normunet_unpack_bwd", _dims(c), c["n"]
    seed = hash_case(c)
    gout, q, st = _rand(seed + 4, n, h, w, 2), _rand(seed + 5, n, 2, pad16(h), pad16(w)), _stats(seed + 6, n)
    gq, ds = vjp(lambda q_, s_: ref_unpack(q_, s_, (h, w)), [q.double(), st.double()], [gout.double()])

    def body(k):
        g, qd, sd, o, dso = k.inp(gout), k.inp(q), k.inp(st), k.out(q.shape), k.out((n, 2, 2))
        check(L().cine_normunet_unpack_bwd(g.data_ptr(), qd.data_ptr(), sd.data_ptr(), o.ptr(), dso.ptr(), n, h, w, stream()), name)
        return [o.t, dso.t]
    o, dso = at_offsets(dev, OFFS, body, name)
    _record(name, peak_err(o, gq), BAR, case_id(c))
    zero_frame(o, wins16(h, w), name)
    # dstats are dot products: against their cancellation-free scale sum |gout| and sum |gout q|
    qin = q.double()[:, :, split16(h)[1]:split16(h)[1] + h, split16(w)[1]:split16(w)[1] + w]
    gch = gout.double().movedim(-1, 1)
    scale = torch.stack([gch.abs().sum(dim=(2, 3)), (gch * qin).abs().sum(dim=(2, 3))], dim=2)
    _record(name + " dstats", float(((dso.double() - ds).abs() / scale).max()), BAR, case_id(c))
    q0, g0 = _rand(seed + 7, n, 2, h, w), gout

    def plain(k):
        g, qd, o = k.inp(g0), k.inp(q0), k.out(q0.shape)
        check(L().cine_normunet_unpack_bwd(g.data_ptr(), qd.data_ptr(), None, o.ptr(), None, n, h, w, stream()), name)
        return [o.t]
    o, = at_offsets(dev, OFFS, plain, name + " stats=NULL")
    assert same_bits(o, ref_pack(g0, False)[0]), f"{name} with NULL stats is not the plain repack"


@gpu
@pytest.mark.parametrize("c", N_CASES, ids=case_id)
def test_normunet_pack_bwd(dev, c):
    """Planes under 16 elements are judged against norm_bwd_scale where it exceeds the reference's peak: the exact gradient of a
    two-element plane's term is 0, and float32 leaves the rounding of terms of size |gp| / std."""
    name, (h, w), n = "cine_normunet_pack_bwd", _dims(c), c["n"]
    d = nv_ref(c)
    seed = hash_case(c)
    gp, ds = _rand(seed + 8, *d["p"].shape), _rand(seed + 9, n, 2, 2)
    gz, = vjp(lambda x_: ref_pack(x_, True), [d["x"].double()], [gp.double(), ds.double()])
    p32, s32 = d["p"].float(), d["s"].float()
    scale = float(gz.abs().max())
    if h * w < TINY:
        scale = max(scale, norm_bwd_scale(gp.double(), d["p"], d["s"], ds.double(), h * w))

    def body(k):
        g, p, s, dd, o = k.inp(gp), k.inp(p32), k.inp(s32), k.inp(ds), k.out((n, h, w, 2))
        check(L().cine_normunet_pack_bwd(g.data_ptr(), p.data_ptr(), s.data_ptr(), dd.data_ptr(), o.ptr(), n, h, w, stream()), name)
        return [o.t]
    o, = at_offsets(dev, OFFS, body, name)
    _record(name, peak_err(o, gz, scale), BAR, case_id(c))
    if c["fam"] == "rand":
        g0 = _rand(seed + 10, n, 2, h, w)

        def plain(k):
            g, o = k.inp(g0), k.out((n, h, w, 2))
            check(L().cine_normunet_pack_bwd(g.data_ptr(), None, None, None, o.ptr(), n, h, w, stream()), name)
            return [o.t]
        o, = at_offsets(dev, OFFS, plain, name + " stats=NULL")
        assert same_bits(o, ref_unpack(g0, None, (h, w))), f"{name} with NULL stats is not the inverse repack"


# ------------------------------------------------------------------ R: the rotations
def _r_shapes(c):
    b, t, h, w, norm = c["b"], c["t"], c["h"], c["w"], c["norm"]
    (wp, _), (hp, _), (tp, _) = split16(w, norm), split16(h, norm), split16(t, norm)
    return (b * h, 2, wp, tp), (b * w, 2, hp, tp)


def _opt(t):
    return None if t is None else t.data_ptr()


@gpu
def test_rotation_size_functions(dev):
    lib = L()
    for c in R_CASES:
        want = c["b"] * c["t"] * c["h"] * c["w"] * 8
        assert lib.cine_xfyf_ws_bytes(c["b"], c["t"], c["h"], c["w"]) == want == lib.cine_xfyf_bwd_ws_bytes(c["b"], c["t"], c["h"], c["w"])
    for c in x_cases("pack"):
        assert lib.cine_xpd_ws_bytes(c["b"], c["t"], c["h"], c["w"], c["n"]) == c["b"] * c["t"] * c["h"] * c["w"] * (c["n"] + 1) * 8


def _xfyf_pack_body(c, img, keep_ws=None):
    b, t, h, w, xf, norm = (c[k] for k in ("b", "t", "h", "w", "xf", "norm"))
    sx, sy = _r_shapes(c)

    def body(k):
        x, px, py, m = k.inp(img), k.out(sx), k.out(sy), k.out((b, h, w, 2))
        stx, sty = (k.out((b * h, 2, 2)), k.out((b * w, 2, 2))) if norm else (None, None)
        ws = k.ws(L().cine_xfyf_ws_bytes(b, t, h, w))
        check(L().cine_xfyf_pack(x.data_ptr(), px.ptr(), py.ptr(), stx and stx.ptr(), sty and sty.ptr(), m.ptr(), b, t, h, w, xf, norm,
                                 ws.ptr(), ws.nbytes, stream()), "cine_xfyf_pack")
        if keep_ws is not None:
            keep_ws.append(ws.buf[:ws.nbytes].clone().view(torch.float32).view(b, h, w, t, 2).cpu())
        return [px.t, py.t, m.t] + ([stx.t, sty.t] if norm else [])
    return body


@gpu
@pytest.mark.parametrize("c", R_CASES, ids=case_id)
def test_xfyf_pack(dev, c):
    d = r_ref(c)
    pxf, pyf, sxf, syf, mean = d["out"]
    got = at_offsets(dev, OFFS, _xfyf_pack_body(c, d["img"]), "cine_xfyf_pack")
    case = case_id(c)
    _record("cine_xfyf_pack", max(peak_err(got[0], pxf), peak_err(got[1], pyf)), BAR, case)
    _record("cine_xfyf_pack mean_img", peak_err(got[2], mean), BAR, case)
    if c["norm"]:
        zero_frame(got[0], wins16(c["w"], c["t"]), "cine_xfyf_pack planes_xf")
        zero_frame(got[1], wins16(c["h"], c["t"]), "cine_xfyf_pack planes_yf")
        # the rotated planes have zero temporal mean, so their group means are rounding residue of the planes' own size: measured
        # against the peak std (the scale of the values that were averaged); the stds against their own peak
        for g, r in ((got[3], sxf), (got[4], syf)):
            _record("cine_xfyf_pack stats mean", float((g.double()[..., 0] - r[..., 0]).abs().max() / r[..., 1].abs().max()), BAR, case)
            _mean_std_record("cine_xfyf_pack stats", g, r, case, means=False)


@gpu
@pytest.mark.parametrize("c", [c for c in R_CASES if c["norm"]], ids=case_id)
def test_xfyf_pack_without_the_norm_gives_the_rotation_the_norm_normalises(dev, c):
    """The workspace holds the rotated frames X (b, h, w, t): the same bits with the norm on and off, the norm-off planes are X's bits
    re-ordered, and the temporal mean image is the same."""
    img = r_ref(c)["img"]
    b, t, h, w = c["b"], c["t"], c["h"], c["w"]
    ws_on, ws_off = [], []
    on = twice(dev, 0, _xfyf_pack_body(c, img, ws_on), "cine_xfyf_pack")
    off = twice(dev, 0, _xfyf_pack_body(dict(c, norm=0), img, ws_off), "cine_xfyf_pack norm=0")
    X = ws_off[0]
    assert same_bits(ws_on[0], X) and same_bits(on[2], off[2])
    assert same_bits(off[0], X.reshape(b * h, w, t, 2).permute(0, 3, 1, 2).contiguous())
    assert same_bits(off[1], X.permute(0, 2, 1, 3, 4).reshape(b * w, h, t, 2).permute(0, 3, 1, 2).contiguous())


def _r_back_inputs(c):
    b, h, w = c["b"], c["h"], c["w"]
    seed = hash_case(c)
    sx, sy = _r_shapes(c)
    qx, qy, mean = _rand(seed + 11, *sx), _rand(seed + 12, *sy), _rand(seed + 13, b, h, w, 2)
    stx, sty = (_stats(seed + 14, b * h), _stats(seed + 15, b * w)) if c["norm"] else (None, None)
    return qx, qy, stx, sty, mean


def _dbl(*ts):
    return [None if t is None else t.double() for t in ts]


@gpu
@pytest.mark.parametrize("c", R_CASES, ids=case_id)
def test_xfyf_unpack(dev, c):
    b, t, h, w, xf = (c[k] for k in ("b", "t", "h", "w", "xf"))
    qx, qy, stx, sty, mean = _r_back_inputs(c)
    ref = ref_xfyf_unpack(*_dbl(qx, qy, stx, sty, mean), (b, t, h, w), xf)

    def body(k):
        a, bb, s1, s2, m, o = k.inp(qx), k.inp(qy), k.inp(stx), k.inp(sty), k.inp(mean), k.out((b, t, h, w, 2))
        check(L().cine_xfyf_unpack(a.data_ptr(), bb.data_ptr(), _opt(s1), _opt(s2), m.data_ptr(), o.ptr(), b, t, h, w, xf, stream()), "cine_xfyf_unpack")
        return [o.t]
    o, = at_offsets(dev, OFFS, body, "cine_xfyf_unpack")
    _record("cine_xfyf_unpack", peak_err(o, ref), BAR, case_id(c))


@gpu
@pytest.mark.parametrize("c", R_CASES, ids=case_id)
def test_xfyf_unpack_bwd(dev, c):
    name = "cine_xfyf_unpack_bwd"
    b, t, h, w, xf, norm = (c[k] for k in ("b", "t", "h", "w", "xf", "norm"))
    qx, qy, stx, sty, mean = _r_back_inputs(c)
    gout = _rand(hash_case(c) + 16, b, t, h, w, 2)
    if norm:
        gr = vjp(lambda a, bb, s1, s2, m: ref_xfyf_unpack(a, bb, s1, s2, m, (b, t, h, w), xf), _dbl(qx, qy, stx, sty, mean), [gout.double()])
    else:
        g3 = vjp(lambda a, bb, m: ref_xfyf_unpack(a, bb, None, None, m, (b, t, h, w), xf), _dbl(qx, qy, mean), [gout.double()])
        gr = [g3[0], g3[1], None, None, g3[2]]

    def body(k):
        g, a, bb, s1, s2 = k.inp(gout), k.inp(qx), k.inp(qy), k.inp(stx), k.inp(sty)
        ox, oy, gm = k.out(qx.shape), k.out(qy.shape), k.out((b, h, w, 2))
        dx, dy = (k.out((b * h, 2, 2)), k.out((b * w, 2, 2))) if norm else (None, None)
        ws = k.ws(L().cine_xfyf_bwd_ws_bytes(b, t, h, w))
        check(L().cine_xfyf_unpack_bwd(g.data_ptr(), a.data_ptr(), bb.data_ptr(), _opt(s1), _opt(s2), ox.ptr(), oy.ptr(), dx and dx.ptr(), dy and dy.ptr(),
                                       gm.ptr(), b, t, h, w, xf, ws.ptr(), ws.nbytes, stream()), name)
        return [ox.t, oy.t, gm.t] + ([dx.t, dy.t] if norm else [])
    got = at_offsets(dev, OFFS, body, name)
    case = case_id(c)
    _record(name, max(peak_err(got[0], gr[0]), peak_err(got[1], gr[1])), BAR, case)
    _record(name + " gmean", peak_err(got[2], gr[4]), BAR, case)
    if norm:
        zero_frame(got[0], wins16(w, t), name)
        zero_frame(got[1], wins16(h, t), name)
        # dstats = sums of g and g q over a plane, g = 0.5 x the transformed gout: against the cancellation-free scale of those sums
        for o, ref, gq, q, st, dims in ((got[3], gr[2], gr[0], qx, stx, (w, t)), (got[4], gr[3], gr[1], qy, sty, (h, t))):
            sl = (slice(None), slice(None)) + tuple(slice(split16(v)[1], split16(v)[1] + v) for v in dims)
            g = gq[sl] / st.double()[:, :, 1, None, None]                       # gq = g std inside the window
            scale = torch.stack([g.abs().sum(dim=(2, 3)), (g * q.double()[sl]).abs().sum(dim=(2, 3))], dim=2)
            _record(name + " dstats", float(((o.double() - ref).abs() / scale).max()), BAR, case)


@gpu
@pytest.mark.parametrize("c", R_CASES, ids=case_id)
def test_xfyf_pack_bwd(dev, c):
    """Plane sets with fewer than 16 elements per plane: against norm_bwd_scale where it exceeds the reference's peak (see the module)."""
    name = "cine_xfyf_pack_bwd"
    b, t, h, w, xf, norm = (c[k] for k in ("b", "t", "h", "w", "xf", "norm"))
    d = r_ref(c)
    pxf, pyf, sxf, syf, _ = d["out"]
    seed = hash_case(c)
    gpx, gpy, gmean = _rand(seed + 17, *pxf.shape), _rand(seed + 18, *pyf.shape), _rand(seed + 19, b, h, w, 2)
    dsx, dsy = (_rand(seed + 20, b * h, 2, 2), _rand(seed + 21, b * w, 2, 2)) if norm else (None, None)
    gimg, = vjp(lambda x_: ref_xfyf_pack(x_, xf, norm), [d["img"].double()], _dbl(gpx, gpy, dsx, dsy, gmean))
    scale = float(gimg.abs().max())
    if norm:
        for gp, p, s, ds, cnt in ((gpx, pxf, sxf, dsx, w * t), (gpy, pyf, syf, dsy, h * t)):
            if cnt < TINY:
                scale = max(scale, norm_bwd_scale(gp.double(), p, s, ds.double(), cnt))
    f32 = lambda v: None if v is None else v.float()

    def body(k):
        a, bb, p1, p2, s1, s2, d1, d2, gm = (k.inp(v) for v in (gpx, gpy, f32(pxf) if norm else None, f32(pyf) if norm else None, f32(sxf), f32(syf), dsx, dsy, gmean))
        o, ws = k.out((b, t, h, w, 2)), k.ws(L().cine_xfyf_bwd_ws_bytes(b, t, h, w))
        check(L().cine_xfyf_pack_bwd(a.data_ptr(), bb.data_ptr(), _opt(p1), _opt(p2), _opt(s1), _opt(s2), _opt(d1), _opt(d2), gm.data_ptr(), o.ptr(),
                                     b, t, h, w, xf, ws.ptr(), ws.nbytes, stream()), name)
        return [o.t]
    o, = at_offsets(dev, OFFS, body, name)
    _record(name, peak_err(o, gimg, scale), BAR, case_id(c))


# ------------------------------------------------------------------ X: the XPD buffers
def _x_shapes(c, chans):
    b, t, h, w, ns = c["b"], c["t"], c["h"], c["w"], c["ns"]
    return (b * h, chans, mw_pad(w, ns)[0], mw_pad(t, ns)[0]), (b * w, chans, mw_pad(h, ns)[0], mw_pad(t, ns)[0])


@gpu
@pytest.mark.parametrize("c", x_cases("pack"), ids=case_id)
def test_xpd_pack(dev, c):
    name = "cine_xpd_pack"
    b, t, h, w, n, ns, xf = (c[k] for k in ("b", "t", "h", "w", "n", "ns", "xf"))
    seed = hash_case(c)
    buf, extra = _rand(seed, b, t, h, w, 2 * n), _rand(seed + 1, b, t, h, w, 2)
    pxf, pyf, mean = ref_xpd_pack(buf.double(), extra.double(), n, ns, xf)

    def body(k):
        a, e, px, py, m = k.inp(buf), k.inp(extra), k.out(pxf.shape), k.out(pyf.shape), k.out(mean.shape)
        ws = k.ws(L().cine_xpd_ws_bytes(b, t, h, w, n))
        check(L().cine_xpd_pack(a.data_ptr(), e.data_ptr(), px.ptr(), py.ptr(), m.ptr(), b, t, h, w, n, ns, xf, ws.ptr(), ws.nbytes, stream()), name)
        return [px.t, py.t, m.t]
    got = at_offsets(dev, OFFS, body, name)
    _record(name, max(peak_err(got[0], pxf), peak_err(got[1], pyf)), BAR, case_id(c))
    _record(name + " mean", peak_err(got[2], mean), BAR, case_id(c))
    zero_frame(got[0], wins_mw(ns, w, t), name)
    zero_frame(got[1], wins_mw(ns, h, t), name)


def _x_back_inputs(c):
    seed = hash_case(c)
    sx, sy = _x_shapes(c, 2 * c["n"])
    return _rand(seed + 2, *sx), _rand(seed + 3, *sy), _rand(seed + 4, c["b"], c["h"], c["w"], c["n"] + 1, 2)


@gpu
@pytest.mark.parametrize("c", x_cases("unpack"), ids=case_id)
def test_xpd_unpack(dev, c):
    name = "cine_xpd_unpack"
    b, t, h, w, n, ns, xf = (c[k] for k in ("b", "t", "h", "w", "n", "ns", "xf"))
    qx, qy, mean = _x_back_inputs(c)
    ref = ref_xpd_unpack(*_dbl(qx, qy, mean), (b, t, h, w), n, ns, xf)

    def body(k):
        a, bb, m, o = k.inp(qx), k.inp(qy), k.inp(mean), k.out(ref.shape)
        check(L().cine_xpd_unpack(a.data_ptr(), bb.data_ptr(), m.data_ptr(), o.ptr(), b, t, h, w, n, ns, xf, stream()), name)
        return [o.t]
    o, = at_offsets(dev, OFFS, body, name)
    _record(name, peak_err(o, ref), BAR, case_id(c))


@gpu
@pytest.mark.parametrize("c", x_cases("unpack_bwd"), ids=case_id)
def test_xpd_unpack_bwd(dev, c):
    name = "cine_xpd_unpack_bwd"
    b, t, h, w, n, ns, xf = (c[k] for k in ("b", "t", "h", "w", "n", "ns", "xf"))
    qx, qy, mean = _x_back_inputs(c)
    gout = _rand(hash_case(c) + 5, b, t, h, w, 2 * n)
    gx, gy, gm = vjp(lambda a, bb, m: ref_xpd_unpack(a, bb, m, (b, t, h, w), n, ns, xf), _dbl(qx, qy, mean), [gout.double()])

    def body(k):
        g, ox, oy, om = k.inp(gout), k.out(qx.shape), k.out(qy.shape), k.out(mean.shape)
        check(L().cine_xpd_unpack_bwd(g.data_ptr(), ox.ptr(), oy.ptr(), om.ptr(), b, t, h, w, n, ns, xf, stream()), name)
        return [ox.t, oy.t, om.t]
    got = at_offsets(dev, OFFS, body, name)
    _record(name, max(peak_err(got[0], gx), peak_err(got[1], gy)), BAR, case_id(c))
    _record(name + " gmean", peak_err(got[2], gm), BAR, case_id(c))
    zero_frame(got[0], wins_mw(ns, w, t), name)
    zero_frame(got[1], wins_mw(ns, h, t), name)
    assert not bool(got[2][..., n, :].any()), f"{name}: the gradient of the dropped channel's mean is not 0"


@gpu
@pytest.mark.parametrize("c", x_cases("pack_bwd"), ids=case_id)
def test_xpd_pack_bwd(dev, c):
    name = "cine_xpd_pack_bwd"
    b, t, h, w, n, ns, xf = (c[k] for k in ("b", "t", "h", "w", "n", "ns", "xf"))
    seed = hash_case(c)
    sx, sy = _x_shapes(c, 2 * (n + 1))
    gpx, gpy, gmean = _rand(seed + 6, *sx), _rand(seed + 7, *sy), _rand(seed + 8, b, h, w, n + 1, 2)
    buf, extra = torch.zeros(b, t, h, w, 2 * n, dtype=torch.float64), torch.zeros(b, t, h, w, 2, dtype=torch.float64)      # the map is linear
    gb, ge = vjp(lambda a, e: ref_xpd_pack(a, e, n, ns, xf), [buf, extra], _dbl(gpx, gpy, gmean))

    def body(k):
        a, bb, m, ob, oe = k.inp(gpx), k.inp(gpy), k.inp(gmean), k.out(gb.shape), k.out(ge.shape)
        check(L().cine_xpd_pack_bwd(a.data_ptr(), bb.data_ptr(), m.data_ptr(), ob.ptr(), oe.ptr(), b, t, h, w, n, ns, xf, stream()), name)
        return [ob.t, oe.t]
    ob, oe = at_offsets(dev, OFFS, body, name)
    _record(name, peak_err(ob, gb), BAR, case_id(c))
    _record(name + " gextra", peak_err(oe, ge), BAR, case_id(c))


@gpu
@pytest.mark.parametrize("c", CHANLAST_CASES, ids=case_id)
def test_chanlast_pair(dev, c):
    n, C, h, w, ns = (c[k] for k in ("n", "c", "h", "w", "ns"))
    x = _rand(hash_case(c), n, h, w, C)
    ref = ref_chanlast_to_planes(x, ns)

    def fwd(k):
        a, p = k.inp(x), k.out(ref.shape)
        check(L().cine_chanlast_to_planes(a.data_ptr(), p.ptr(), n, C, h, w, ns, stream()), "cine_chanlast_to_planes")
        return [p.t]
    p, = at_offsets(dev, OFFS, fwd, "cine_chanlast_to_planes")
    assert same_bits(p, ref), "cine_chanlast_to_planes is not a zero-padded gather"
    q = _rand(hash_case(c) + 1, *ref.shape)                          # anything on the pad frame: it is dropped

    def back(src):
        def body(k):
            a, y = k.inp(src), k.out(x.shape)
            check(L().cine_planes_to_chanlast(a.data_ptr(), y.ptr(), n, C, h, w, ns, stream()), "cine_planes_to_chanlast")
            return [y.t]
        return body
    y, = at_offsets(dev, OFFS, back(q), "cine_planes_to_chanlast")
    assert same_bits(y, ref_planes_to_chanlast(q, h, w, ns)), "cine_planes_to_chanlast is not a gather"
    y, = at_offsets(dev, OFFS, back(p), "cine_planes_to_chanlast")
    assert same_bits(y, x), "planes_to_chanlast(chanlast_to_planes(x)) does not return x's bits"
    # the pair is adjoint: <A x, q> = <x, A^H q>, exactly the same products
    assert float((p.double() * q.double()).sum()) == pytest.approx(float((x.double() * ref_planes_to_chanlast(q, h, w, ns).double()).sum()), rel=1e-12)
    _record("cine_chanlast_to_planes", 0.0, BAR, case_id(c))
    _record("cine_planes_to_chanlast", 0.0, BAR, case_id(c))


@gpu
@pytest.mark.parametrize("c", EXTRACT_CASES, ids=case_id)
def test_extract_complex(dev, c):
    npix, C, c_re, c_im = (c[k] for k in ("npix", "c", "c_re", "c_im"))
    buf = _rand(hash_case(c), npix, C)

    def body(k):
        a, o = k.inp(buf), k.out((npix, 2))
        check(L().cine_extract_complex(a.data_ptr(), o.ptr(), npix, C, c_re, c_im, stream()), "cine_extract_complex")
        return [o.t]
    o, = at_offsets(dev, OFFS, body, "cine_extract_complex")
    assert same_bits(o, torch.stack([buf[:, c_re], buf[:, c_im]], dim=1))
    _record("cine_extract_complex", 0.0, BAR, case_id(c))


@gpu
@pytest.mark.parametrize("c", REPEAT_CASES, ids=case_id)
def test_repeat_complex(dev, c):
    npix, n = c["npix"], c["n"]
    img = _rand(hash_case(c), npix, 2)

    def body(k):
        a, o = k.inp(img), k.out((npix, 2 * n))
        check(L().cine_repeat_complex(a.data_ptr(), o.ptr(), npix, n, stream()), "cine_repeat_complex")
        return [o.t]
    o, = at_offsets(dev, OFFS, body, "cine_repeat_complex")
    assert same_bits(o, ref_repeat(img, n))
    _record("cine_repeat_complex", 0.0, BAR, case_id(c))


# ------------------------------------------------------------------ E: element-wise
def _away_from_zero(x):
    """|x| >= 0.25 per complex value: the references divide by |x| too."""
    r = x.pow(2).sum(dim=-1, keepdim=True).sqrt()
    return (x * (r + 0.25) / r).contiguous()


@gpu
@pytest.mark.parametrize("n", E_N)
def test_complex_abs_and_its_adjoint(dev, n):
    x, gy = _away_from_zero(_rand(n, n, 2)), _rand(n + 1, n)
    ref = x.double().pow(2).sum(dim=1).sqrt()
    gx, = vjp(lambda v: v.pow(2).sum(dim=1).sqrt(), [x.double()], [gy.double()])

    def fwd(k):
        a, o = k.inp(x), k.out((n,))
        check(L().cine_complex_abs(a.data_ptr(), o.ptr(), n, stream()), "cine_complex_abs")
        return [o.t]
    o, = at_offsets(dev, OFFS, fwd, "cine_complex_abs")
    _record("cine_complex_abs", peak_err(o, ref), BAR, n)

    def bwd(k):
        g, a, o = k.inp(gy), k.inp(x), k.out((n, 2))
        check(L().cine_complex_abs_bwd(g.data_ptr(), a.data_ptr(), o.ptr(), n, stream()), "cine_complex_abs_bwd")
        return [o.t]
    o, = at_offsets(dev, OFFS, bwd, "cine_complex_abs_bwd")
    _record("cine_complex_abs_bwd", peak_err(o, gx), BAR, n)


@gpu
@pytest.mark.parametrize("c", RSS_CASES, ids=case_id)
def test_rss_normalise_bwd(dev, c):
    b, C, h, w = (c[k] for k in ("b", "c", "h", "w"))
    x, gy = _away_from_zero(_rand(hash_case(c), b, C, h, w, 2)), _rand(hash_case(c) + 1, b, C, h, w, 2)
    gx, = vjp(ref_rss_normalise, [x.double()], [gy.double()])

    def body(k):
        g, a, o = k.inp(gy), k.inp(x), k.out(x.shape)
        check(L().cine_rss_normalise_bwd(g.data_ptr(), a.data_ptr(), o.ptr(), b, C, h, w, stream()), "cine_rss_normalise_bwd")
        return [o.t]
    o, = at_offsets(dev, OFFS, body, "cine_rss_normalise_bwd")
    _record("cine_rss_normalise_bwd", peak_err(o, gx), BAR, case_id(c))


# ------------------------------------------------------------------ <A x, y> = <x, A^H y> on the device's own outputs
def _dev_call(dev, fn, ins, out_shapes, ws_bytes=0):
    """One plain call: inputs on the device, zero-filled outputs, a workspace; the outputs on the CPU in float64."""
    ins = [None if t is None else t.to(dev) for t in ins]
    outs = [torch.zeros(s, device=dev) for s in out_shapes]
    ws = torch.zeros(max(ws_bytes, 1), dtype=torch.uint8, device=dev)
    check(fn([_opt(t) for t in ins], [o.data_ptr() for o in outs], ws.data_ptr(), ws_bytes), "adjoint pair")
    torch.cuda.synchronize()
    return [o.double().cpu() for o in outs]


def _adjoint_identity(name, xs, Ax, ys, AHy, case):
    lhs = sum(float((a * y.double()).sum()) for a, y in zip(Ax, ys))
    rhs = sum(float((x.double() * g).sum()) for x, g in zip(xs, AHy))
    scale = sum(float((a * y.double()).abs().sum()) for a, y in zip(Ax, ys))
    _record(name + " <Ax,y>=<x,AHy>", abs(lhs - rhs) / scale, BAR, case)


@gpu
@pytest.mark.parametrize("c", [c for c in R_CASES if not c["norm"]], ids=case_id)
def test_rotations_without_the_norm_are_adjoint_pairs(dev, c):
    lib, st = L(), stream()
    b, t, h, w, xf = (c[k] for k in ("b", "t", "h", "w", "xf"))
    sx, sy = _r_shapes(c)
    seed, wsb = hash_case(c), lib.cine_xfyf_ws_bytes(b, t, h, w)
    img, yx, yy, ym = _rand(seed + 30, b, t, h, w, 2), _rand(seed + 31, *sx), _rand(seed + 32, *sy), _rand(seed + 33, b, h, w, 2)
    Ax = _dev_call(dev, lambda i, o, ws, n: lib.cine_xfyf_pack(i[0], o[0], o[1], None, None, o[2], b, t, h, w, xf, 0, ws, n, st), [img], [sx, sy, (b, h, w, 2)], wsb)
    AHy = _dev_call(dev, lambda i, o, ws, n: lib.cine_xfyf_pack_bwd(i[0], i[1], None, None, None, None, None, None, i[2], o[0], b, t, h, w, xf, ws, n, st),
                    [yx, yy, ym], [(b, t, h, w, 2)], wsb)
    _adjoint_identity("cine_xfyf_pack", [img], Ax, [yx, yy, ym], AHy, case_id(c))
    y = _rand(seed + 34, b, t, h, w, 2)
    Ax = _dev_call(dev, lambda i, o, ws, n: lib.cine_xfyf_unpack(i[0], i[1], None, None, i[2], o[0], b, t, h, w, xf, st), [yx, yy, ym], [(b, t, h, w, 2)])
    AHy = _dev_call(dev, lambda i, o, ws, n: lib.cine_xfyf_unpack_bwd(i[0], i[1], i[2], None, None, o[0], o[1], None, None, o[2], b, t, h, w, xf, ws, n, st),
                    [y, yx, yy], [sx, sy, (b, h, w, 2)], wsb)
    _adjoint_identity("cine_xfyf_unpack", [yx, yy, ym], Ax, [y], AHy, case_id(c))


@gpu
@pytest.mark.parametrize("c", x_cases("pack_bwd"), ids=case_id)
def test_xpd_halves_are_adjoint_pairs(dev, c):
    lib, st = L(), stream()
    b, t, h, w, n, ns, xf = (c[k] for k in ("b", "t", "h", "w", "n", "ns", "xf"))
    seed = hash_case(c)
    sx, sy = _x_shapes(c, 2 * (n + 1))
    buf, extra = _rand(seed + 40, b, t, h, w, 2 * n), _rand(seed + 41, b, t, h, w, 2)
    yx, yy, ym = _rand(seed + 42, *sx), _rand(seed + 43, *sy), _rand(seed + 44, b, h, w, n + 1, 2)
    Ax = _dev_call(dev, lambda i, o, ws, nb: lib.cine_xpd_pack(i[0], i[1], o[0], o[1], o[2], b, t, h, w, n, ns, xf, ws, nb, st), [buf, extra],
                   [sx, sy, (b, h, w, n + 1, 2)], lib.cine_xpd_ws_bytes(b, t, h, w, n))
    AHy = _dev_call(dev, lambda i, o, ws, nb: lib.cine_xpd_pack_bwd(i[0], i[1], i[2], o[0], o[1], b, t, h, w, n, ns, xf, st), [yx, yy, ym],
                    [buf.shape, extra.shape])
    _adjoint_identity("cine_xpd_pack", [buf, extra], Ax, [yx, yy, ym], AHy, case_id(c))
    qx, qy, qm = _x_back_inputs(c)
    y = _rand(seed + 45, b, t, h, w, 2 * n)
    Ax = _dev_call(dev, lambda i, o, ws, nb: lib.cine_xpd_unpack(i[0], i[1], i[2], o[0], b, t, h, w, n, ns, xf, st), [qx, qy, qm], [y.shape])
    AHy = _dev_call(dev, lambda i, o, ws, nb: lib.cine_xpd_unpack_bwd(i[0], o[0], o[1], o[2], b, t, h, w, n, ns, xf, st), [y], [qx.shape, qy.shape, qm.shape])
    _adjoint_identity("cine_xpd_unpack", [qx, qy, qm], Ax, [y], AHy, case_id(c))


# ================================================================== refusals: decided on the host, before any launch
def _swap(args, i, v):
    return args[:i] + (v,) + args[i + 1:]


def _refuse(k, name, args, nulls=(), bad=()):
    """Every pointer of `nulls` NULL in turn -> EINVAL; every (index or {index: value}, code, what) of `bad`."""
    entry = getattr(L(), name)
    for i in nulls:
        refused(lambda: entry(*_swap(args, i, None)), EINVAL, k, f"{name} argument {i} NULL")
    for repl, code, what in bad:
        a = args
        for i, v in repl.items():
            a = _swap(a, i, v)
        refused(lambda: entry(*a), code, k, f"{name} {what}")


@gpu
def test_halves_refusals(dev):
    st, n, h, w, t = stream(), 2, 3, 5, 2
    k = Call(dev, 0)
    x, p, s, ds = k.inp(_rand(1, n, h, w, 2)), k.inp(_rand(2, n, 2, 16, 16)), k.inp(_stats(3, n)), k.inp(_rand(4, n, 2, 2))
    P, S, Y, DS = k.out((n, 2, 16, 16)), k.out((n, 2, 2)), k.out((n, h, w, 2)), k.out((n, 2, 2))
    X, Pi, Si, Di = x.data_ptr(), p.data_ptr(), s.data_ptr(), ds.data_ptr()
    sizes = [({3: 0}, EINVAL, "n=0"), ({4: 0}, EINVAL, "h=0"), ({5: -1}, EINVAL, "w=-1")]
    _refuse(k, "cine_normunet_pack", (X, P.ptr(), S.ptr(), n, h, w, 1, st), (0, 1, 2), sizes + [({4: 1, 5: 1}, EINVAL, "h w = 1")])
    _refuse(k, "cine_normunet_pack", (X, P.ptr(), None, n, h, w, 0, st), (0, 1), [({4: 1, 5: 1}, EINVAL, "h w = 1, norm=0")])
    _refuse(k, "cine_normunet_unpack", (Pi, Si, Y.ptr(), n, h, w, st), (0, 2), sizes + [({3: 65536, 4: 1, 5: 1}, EINVAL, "n=65536")])
    _refuse(k, "cine_normunet_unpack_bwd", (X, Pi, Si, P.ptr(), DS.ptr(), n, h, w, st), (0, 1, 3, 2, 4),            # stats and dstats: both or neither
            [({5: 0}, EINVAL, "n=0"), ({6: 0}, EINVAL, "h=0")])
    _refuse(k, "cine_normunet_pack_bwd", (Pi, Pi, Si, Di, Y.ptr(), n, h, w, st), (0, 4, 1, 3),                       # stats given: planes and dstats too
            [({5: 0}, EINVAL, "n=0"), ({6: 1, 7: 1}, EINVAL, "h w = 1")])
    # 3-D: a volume (n, 2, 3, 5) inside the same buffers
    _refuse(k, "cine_normunet3d_pack", (X, P.ptr(), S.ptr(), 1, t, h, w, 1, st), (0, 1, 2),
            [({3: 0}, EINVAL, "n=0"), ({4: 0}, EINVAL, "t=0"), ({4: 1, 5: 1, 6: 1}, EINVAL, "t h w = 1")])
    _refuse(k, "cine_normunet3d_unpack", (Pi, None, Y.ptr(), 1, t, h, w, st), (0, 2), [({3: 65536, 4: 1, 5: 1, 6: 1}, EINVAL, "n=65536"), ({6: 0}, EINVAL, "w=0")])


@gpu
def test_plain_3d_repack_refuses_65536_samples(dev):
    """The plain repack carries n on grid.y: n = 65 536 volumes of 1 x 1 x 2, every buffer at its full size."""
    n = 65536
    k = Call(dev, 0)
    x, p = k.inp(torch.zeros(n, 1, 1, 2, 2)), k.out((n, 2, 1, 1, 2))
    refused(lambda: L().cine_normunet3d_pack(x.data_ptr(), p.ptr(), None, n, 1, 1, 2, 0, stream()), EINVAL, k, "cine_normunet3d_pack n=65536, norm=0")


def _r_operands(dev, b, t, h, w, zeros=False):
    k = Call(dev, 0)
    mk = (lambda s, *sh: torch.zeros(*sh)) if zeros else _rand
    sx, sy = (b * h, 2, pad16(w), pad16(t)), (b * w, 2, pad16(h), pad16(t))
    a = dict(img=k.inp(mk(1, b, t, h, w, 2)), qx=k.inp(mk(2, *sx)), qy=k.inp(mk(3, *sy)), sx=k.inp(mk(4, b * h, 2, 2) + 1.5), sy=k.inp(mk(5, b * w, 2, 2) + 1.5),
             m=k.inp(mk(6, b, h, w, 2)))
    a = {n_: v.data_ptr() for n_, v in a.items()}
    o = dict(px=k.out(sx), py=k.out(sy), ox=k.out((b * h, 2, 2)), oy=k.out((b * w, 2, 2)), om=k.out((b, h, w, 2)), out=k.out((b, t, h, w, 2)))
    a.update({n_: v.ptr() for n_, v in o.items()})
    nb = L().cine_xfyf_ws_bytes(b, t, h, w)
    a["ws"], a["nb"] = k.ws(nb).ptr(), nb
    return k, a


def _r_calls(a, b, t, h, w, st):
    return {"cine_xfyf_pack": (a["img"], a["px"], a["py"], a["ox"], a["oy"], a["om"], b, t, h, w, 1, 1, a["ws"], a["nb"], st),
            "cine_xfyf_unpack": (a["qx"], a["qy"], a["sx"], a["sy"], a["m"], a["out"], b, t, h, w, 1, st),
            "cine_xfyf_unpack_bwd": (a["img"], a["qx"], a["qy"], a["sx"], a["sy"], a["px"], a["py"], a["ox"], a["oy"], a["om"], b, t, h, w, 1, a["ws"], a["nb"], st),
            "cine_xfyf_pack_bwd": (a["qx"], a["qy"], a["qx"], a["qy"], a["sx"], a["sy"], a["sx"], a["sy"], a["m"], a["out"], b, t, h, w, 1, a["ws"], a["nb"], st)}


R_NULLS = {"cine_xfyf_pack": (0, 1, 2, 3, 4, 5, 12), "cine_xfyf_unpack": (0, 1, 2, 3, 4, 5), "cine_xfyf_unpack_bwd": (0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 15),
           "cine_xfyf_pack_bwd": (0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 15)}         # one statistics pointer alone NULL breaks the all-or-none rules
R_B = {"cine_xfyf_pack": 6, "cine_xfyf_unpack": 6, "cine_xfyf_unpack_bwd": 10, "cine_xfyf_pack_bwd": 10}          # the index of b; t, h, w follow


@gpu
def test_rotation_refusals(dev):
    b, t, h, w, st = 2, 3, 2, 5, stream()
    k, a = _r_operands(dev, b, t, h, w)
    for name, args in _r_calls(a, b, t, h, w, st).items():
        ib = R_B[name]
        bad = [({ib: 0}, EINVAL, "b=0"), ({ib + 1: 1}, EINVAL, "t=1"), ({ib + 2: 0}, EINVAL, "h=0"), ({ib + 3: 0}, EINVAL, "w=0"),
               ({ib + 1: 65}, EUNSUPPORTED if name == "cine_xfyf_pack" else EINVAL, "t=65")]
        if name != "cine_xfyf_unpack":
            bad.append(({len(args) - 2: a["nb"] - 1}, EWORKSPACE, "workspace one byte short"))
        _refuse(k, name, args, R_NULLS[name], bad)
    entry = L().cine_xfyf_pack_bwd
    args = _r_calls(a, b, t, h, w, st)["cine_xfyf_pack_bwd"]
    # both statistics NULL but the planes and dstats given is the plain repack, accepted; stats given with every dstats NULL is not
    refused(lambda: entry(*_swap(_swap(args, 6, None), 7, None)), EINVAL, k, "cine_xfyf_pack_bwd stats without dstats")
    entry = L().cine_xfyf_unpack_bwd
    args = _r_calls(a, b, t, h, w, st)["cine_xfyf_unpack_bwd"]
    refused(lambda: entry(*_swap(_swap(args, 7, None), 8, None)), EINVAL, k, "cine_xfyf_unpack_bwd stats without dstats")
    refused(lambda: entry(*_swap(_swap(args, 3, None), 4, None)), EINVAL, k, "cine_xfyf_unpack_bwd dstats without stats")


@gpu
def test_rotations_refuse_65536_batches(dev):
    """b rides on grid.y (grid.z in the unpack): b = 65 536 images of t = 2, h = w = 1, every buffer at its full size.  cine_xfyf_unpack
    also carries h on grid.y."""
    b, t, h, w, st = 65536, 2, 1, 1, stream()
    k, a = _r_operands(dev, b, t, h, w, zeros=True)
    for name, args in _r_calls(a, b, t, h, w, st).items():
        refused(lambda: getattr(L(), name)(*args), EINVAL, k, f"{name} b=65536")
    args = _r_calls(a, 1, t, b, w, st)["cine_xfyf_unpack"]              # the same buffers as (1, 2, 65536, 1)
    refused(lambda: L().cine_xfyf_unpack(*args), EINVAL, k, "cine_xfyf_unpack h=65536")


def _x_operands(dev, b, t, h, w, n, ns, zeros=False):
    k = Call(dev, 0)
    mk = (lambda s, *sh: torch.zeros(*sh)) if zeros else _rand
    c = dict(b=b, t=t, h=h, w=w, ns=ns)
    sx, sy = _x_shapes(c, 2 * (n + 1))                                  # 2 (n + 1) channels: large enough for the 2n-channel planes too
    a = dict(buf=k.inp(mk(1, b, t, h, w, 2 * n)), extra=k.inp(mk(2, b, t, h, w, 2)), qx=k.inp(mk(3, *sx)), qy=k.inp(mk(4, *sy)), m=k.inp(mk(5, b, h, w, n + 1, 2)))
    a = {n_: v.data_ptr() for n_, v in a.items()}
    o = dict(px=k.out(sx), py=k.out(sy), om=k.out((b, h, w, n + 1, 2)), out=k.out((b, t, h, w, 2 * n)), oe=k.out((b, t, h, w, 2)))
    a.update({n_: v.ptr() for n_, v in o.items()})
    nb = L().cine_xpd_ws_bytes(b, t, h, w, n)
    a["ws"], a["nb"] = k.ws(nb).ptr(), nb
    return k, a


def _x_calls(a, b, t, h, w, n, ns, st):
    return {"cine_xpd_pack": (a["buf"], a["extra"], a["px"], a["py"], a["om"], b, t, h, w, n, ns, 1, a["ws"], a["nb"], st),
            "cine_xpd_unpack": (a["qx"], a["qy"], a["m"], a["out"], b, t, h, w, n, ns, 1, st),
            "cine_xpd_unpack_bwd": (a["buf"], a["px"], a["py"], a["om"], b, t, h, w, n, ns, 1, st),
            "cine_xpd_pack_bwd": (a["qx"], a["qy"], a["m"], a["out"], a["oe"], b, t, h, w, n, ns, 1, st)}


X_NULLS = {"cine_xpd_pack": (0, 1, 2, 3, 4, 12), "cine_xpd_unpack": (0, 1, 2, 3), "cine_xpd_unpack_bwd": (0, 1, 2, 3), "cine_xpd_pack_bwd": (0, 1, 2, 3, 4)}
X_B = {"cine_xpd_pack": 5, "cine_xpd_unpack": 4, "cine_xpd_unpack_bwd": 4, "cine_xpd_pack_bwd": 5}
# the first tile (t, n_primal) each guard refuses
X_FIRST_REFUSED = {"cine_xpd_pack": [(16, 15), (18, 14)], "cine_xpd_unpack": [(18, 15)], "cine_xpd_unpack_bwd": [(18, 15)], "cine_xpd_pack_bwd": [(8, 15), (10, 13)]}


@gpu
def test_xpd_refusals(dev):
    """Sizes, NULLs, a workspace one byte short and the first LDS tile each guard refuses; the buffers are sized for t = 18, n_primal = 15
    on a 2 x 3 plane, so every refused call would have stayed inside them."""
    b, t, h, w, n, ns, st = 1, 18, 2, 3, 15, 1, stream()
    k, a = _x_operands(dev, b, t, h, w, n, ns)
    for name, args in _x_calls(a, b, 3, h, w, 2, ns, st).items():
        ib = X_B[name]
        bad = [({ib: 0}, EINVAL, "b=0"), ({ib + 1: 1}, EINVAL, "t=1"), ({ib + 1: 65}, EINVAL, "t=65"), ({ib + 2: 0}, EINVAL, "h=0"), ({ib + 3: 0}, EINVAL, "w=0"),
               ({ib + 4: 0}, EINVAL, "n_primal=0")]
        bad += [({ib + 1: tt, ib + 4: nn}, EUNSUPPORTED, f"LDS tile ({tt}, {nn})") for tt, nn in X_FIRST_REFUSED[name]]
        if name != "cine_xpd_unpack":                                  # the inference unpack takes any n_primal whose tile fits
            bad.append(({ib + 4: 16}, EINVAL, "n_primal=16"))
        if name == "cine_xpd_pack":
            bad.append(({13: L().cine_xpd_ws_bytes(b, 3, h, w, 2) - 1}, EWORKSPACE, "workspace one byte short"))
        _refuse(k, name, args, X_NULLS[name], bad)


@gpu
def test_xpd_halves_refuse_65536_batches(dev):
    b, t, h, w, n, ns, st = 65536, 2, 1, 1, 1, 0, stream()
    k, a = _x_operands(dev, b, t, h, w, n, ns, zeros=True)
    for name, args in _x_calls(a, b, t, h, w, n, ns, st).items():
        refused(lambda: getattr(L(), name)(*args), EINVAL, k, f"{name} b=65536")
    for name in ("cine_xpd_unpack", "cine_xpd_unpack_bwd"):             # h on grid.y: the same buffers as (1, 2, 65536, 1)
        args = _x_calls(a, 1, t, b, w, n, ns, st)[name]
        refused(lambda: getattr(L(), name)(*args), EINVAL, k, f"{name} h=65536")


@gpu
def test_buffer_and_element_wise_refusals(dev):
    st, n, C, h, w = stream(), 65536, 1, 1, 1
    k = Call(dev, 0)
    x, o = k.inp(torch.zeros(n, 4) + 1.0), k.out((n, 4))
    X, O = x.data_ptr(), o.ptr()
    for name in ("cine_chanlast_to_planes", "cine_planes_to_chanlast"):
        _refuse(k, name, (X, O, 2, 2, 3, 5, 1, st), (0, 1), [({2: 0}, EINVAL, "n=0"), ({3: 0}, EINVAL, "c=0"), ({4: 0}, EINVAL, "h=0"), ({5: 0}, EINVAL, "w=0"),
                                                            ({2: n, 3: C, 4: h, 5: w, 6: 0}, EINVAL, "n=65536")])
    _refuse(k, "cine_extract_complex", (X, O, 5, 3, 0, 1, st), (0, 1), [({2: 0}, EINVAL, "npix=0"), ({3: 0}, EINVAL, "c=0"), ({4: 3}, EINVAL, "c_re=c"),
                                                                       ({4: -1}, EINVAL, "c_re=-1"), ({5: 3}, EINVAL, "c_im=c"), ({5: -1}, EINVAL, "c_im=-1")])
    _refuse(k, "cine_repeat_complex", (X, O, 5, 3, st), (0, 1), [({2: 0}, EINVAL, "npix=0"), ({3: 0}, EINVAL, "n=0")])
    _refuse(k, "cine_complex_abs", (X, O, 5, st), (0, 1), [({2: -1}, EINVAL, "n=-1")])
    _refuse(k, "cine_complex_abs_bwd", (X, X, O, 5, st), (0, 1, 2), [({3: -1}, EINVAL, "n=-1")])
    _refuse(k, "cine_rss_normalise_bwd", (X, X, O, 1, 2, 3, 5, st), (0, 1, 2), [({3: 0}, EINVAL, "b=0"), ({4: 0}, EINVAL, "c=0"), ({5: 0}, EINVAL, "h=0"), ({6: 0}, EINVAL, "w=0"),
                                                                              ({3: n, 4: 2, 5: 1, 6: 1}, EINVAL, "b=65536")])
