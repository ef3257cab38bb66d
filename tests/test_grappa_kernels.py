"""cine_grappa_offsets, cine_grappa_gram, cine_grappa_weights and cine_grappa_apply through ctypes against float64
(tests/grappa_reference.py), the contract of include/cine_hip.h.  The bars are derived, not tuned:

gram     each component of each entry within n_pos 2^-52 sum |terms| of complex128 numpy on the same float32 input: the bound of a
         float64 sum of n_pos exact products.  G - G^H and the diagonal's imaginary part are exactly zero.
weights  max |W_dev - W_ref| <= 8 2^-24 max |W_ref|, W_ref from numpy.linalg.solve in complex128 on the same G: one rounding to
         complex64 costs 2^-24, the float64 forward error is about cond ns 2^-52 with cond <= ns / lam, which stays below 1e-7.
apply    each output component within (2 ns + 1) 2^-24 sum |w| |x| of float64: the bound of a 2 ns-term fp32 chain.
"""
import numpy as np
import pytest
import torch

import grappa_reference as ref
from kernel_sweep import (EINVAL, EUNSUPPORTED, EWORKSPACE, Call, GuardedInt, L, at_offsets, case_id, hash_case, refused, same_bits, stream, sweep,
                          twice)

pytestmark = pytest.mark.gpu

KERNELS = [(2, 3), (2, 5), (4, 5), (4, 7)]


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "-m gpu tests need an MI355X"
    return torch.device("cuda:0")


def pairs(z):
    """complex numpy -> float32 (..., 2) torch."""
    z = np.asarray(z)
    return torch.from_numpy(np.stack((z.real, z.imag), -1).astype(np.float32))


def cplx(t):
    """float (..., 2) torch -> complex128 numpy."""
    a = t.detach().cpu().numpy().astype(np.float64)
    return a[..., 0] + 1j * a[..., 1]


# ================================================================== offsets
def offsets_case(t, h, R, seed):
    """A (t, h) mask and what the rule gives: frame f has the residue (f + seed) mod R; with five frames, frame 1 loses a lattice row
    (offset -1 unless another residue is complete), frame 2 is fully sampled, frame 3 carries an ACS block."""
    offs = [(f + seed) % R for f in range(t)]
    mask = ref.lattice_mask(t, h, R, offsets=offs)
    if t == 5:
        mask[1, offs[1]] = 0
        mask[2, :] = 1
        lo = h // 2 - min(4, h) // 2
        mask[3, lo:lo + min(4, h)] = 1
    return mask, ref.offsets(mask, R)


def run_offsets(dev, mask, R):
    t, h = mask.shape
    m = torch.from_numpy(mask).to(dev)
    off, status = GuardedInt(t, dev, fill=-7), GuardedInt(t, dev, fill=-7)
    assert L().cine_grappa_offsets(m.data_ptr(), off.ptr(), status.ptr(), t, h, R, stream()) == 0, L().cine_last_error()
    torch.cuda.synchronize()
    assert off.intact() and status.intact() and torch.equal(m.cpu(), torch.from_numpy(mask))
    return off.t.cpu().numpy(), status.t.cpu().numpy()


@pytest.mark.parametrize("R", [2, 3, 8])
@pytest.mark.parametrize("hsel", ["R", "R+1", 13, 48])
@pytest.mark.parametrize("t", [1, 5])
def test_offsets(dev, t, hsel, R):
    h = {"R": R, "R+1": R + 1}.get(hsel, hsel)
    for seed in range(R if t == 1 else 2):                                 # t = 1: every residue as the answer
        mask, (want_off, want_status) = offsets_case(t, h, R, seed)
        off, status = run_offsets(dev, mask, R)
        assert off.dtype == np.int32 and off.tolist() == want_off.tolist(), (mask, off, want_off)
        assert status.tolist() == want_status.tolist()
        if t == 5:
            assert off[2] == 0 and status[2] == 0                          # fully sampled
            if h > R + 1:
                assert off[1] == -1 and status[1] == 1                     # no lattice
        again, _ = run_offsets(dev, mask, R)
        assert again.tolist() == off.tolist()


def test_offsets_refusals(dev):
    t, h, R = 3, 12, 3
    m = torch.from_numpy(ref.lattice_mask(t, h, R)).to(dev)
    k = Call(dev, 0)
    off, status = GuardedInt(t, dev), GuardedInt(t, dev)
    k.outs += [off, status]
    good = [m.data_ptr(), off.ptr(), status.ptr(), t, h, R]
    for i in range(3):
        args = good[:i] + [None] + good[i + 1:]
        refused(lambda: L().cine_grappa_offsets(*args, stream()), EINVAL, k, "cine_grappa_offsets null pointer")
    for bad in ([m.data_ptr(), off.ptr(), off.ptr(), t, h, R], good[:3] + [0, h, R], good[:3] + [t, 0, R], good[:5] + [1], good[:5] + [9],
                [m.data_ptr(), off.ptr() + 2, status.ptr(), t, h, R]):
        refused(lambda: L().cine_grappa_offsets(*bad, stream()), EINVAL, k, f"cine_grappa_offsets {bad[3:]}")


# ================================================================== gram
def gram_cases():
    axes = {"c": [1, 3, 8, 17, 32], "kernel": [0, 1, 2, 3], "R": [2, 3, 5, 8], "hc": ["span", "span+1", "24"], "w": ["kx", "kx+1", "40", "67"]}
    out = []
    for case in sweep(20251, axes, 40):
        ky, kx = KERNELS[case["kernel"]]
        g = ref.geom(case["c"], case["R"], ky, kx)
        assert g["n_aug"] <= 1152
        hc = {"span": g["span"], "span+1": g["span"] + 1, "24": max(24, g["span"])}[case["hc"]]
        w = {"kx": kx, "kx+1": kx + 1, "40": 40, "67": 67}[case["w"]]
        out.append({"c": case["c"], "ky": ky, "kx": kx, "R": case["R"], "hc": hc, "w": w})
    return out


def call_gram(k, cal, c, hc, w, R, ky, kx, past256=None, ws_bytes=None):
    n = ref.geom(c, R, ky, kx)["n_aug"]
    need = L().cine_grappa_gram_ws_bytes(c, hc, w, R, ky, kx)
    assert need == hc * w * c * 16
    d_cal = k.inp(cal)
    out = k.out64(2 * n * n)
    ws = k.ws(need if ws_bytes is None else ws_bytes, past256)
    code = L().cine_grappa_gram(d_cal.data_ptr(), out.ptr(), ws.ptr(), ws.nbytes, c, hc, w, R, ky, kx, stream())
    return code, out


@pytest.mark.parametrize("case", gram_cases(), ids=case_id)
def test_gram_against_complex128(dev, case):
    c, ky, kx, R, hc, w = (case[x] for x in ("c", "ky", "kx", "R", "hc", "w"))
    rs = np.random.RandomState(hash_case(case))
    cal = (rs.standard_normal((c, hc, w)) + 1j * rs.standard_normal((c, hc, w))).astype(np.complex64)
    n = ref.geom(c, R, ky, kx)["n_aug"]

    def body(k):
        code, out = call_gram(k, pairs(cal), c, hc, w, R, ky, kx)
        assert code == 0, L().cine_last_error()
        return [out.t]

    got = twice(dev, 0, body, "cine_grappa_gram")[0].numpy().reshape(n, n, 2)      # the same bits on a second call, sentinels intact
    G = got[..., 0] + 1j * got[..., 1]
    want = ref.gram(cal, R, ky, kx)
    b_re, b_im = ref.gram_bounds(cal, R, ky, kx)
    e_re, e_im = np.abs(G.real - want.real), np.abs(G.imag - want.imag)
    worst = max(float((e_re / np.maximum(b_re, 1e-300)).max()), float((e_im / np.maximum(b_im, 1e-300)).max()))
    print(f"{case_id(case)}: n_aug {n}, worst error {worst:.3f} of its bound")
    assert (e_re <= b_re).all() and (e_im <= b_im).all()
    assert (G == G.conj().T).all() and (np.diagonal(G).imag == 0).all()            # exactly Hermitian, a real diagonal
    # a workspace 8 bytes past a 16-byte boundary: the entry demands 16-byte alignment and refuses the placement
    k = Call(dev, 0)
    d_cal = k.inp(pairs(cal))
    out = k.out64(2 * n * n)
    ws = k.ws(L().cine_grappa_gram_ws_bytes(c, hc, w, R, ky, kx), past256=8)
    refused(lambda: L().cine_grappa_gram(d_cal.data_ptr(), out.ptr(), ws.ptr(), ws.nbytes, c, hc, w, R, ky, kx, stream()), EINVAL, k,
            "cine_grappa_gram workspace off its alignment")


def test_gram_refusals(dev):
    c, hc, w, R, ky, kx = 3, 12, 9, 3, 2, 5
    cal = pairs(np.ones((c, hc, w), np.complex64))
    k = Call(dev, 0)
    d_cal = k.inp(cal)
    n = ref.geom(c, R, ky, kx)["n_aug"]
    out = k.out64(2 * n * n)
    ws = k.ws(1 << 20)
    lib = L()
    good = [d_cal.data_ptr(), out.ptr(), ws.ptr(), ws.nbytes, c, hc, w, R, ky, kx]

    def bad(want, what, **kw):
        names = ["cal", "gram", "ws", "ws_bytes", "c", "hc", "w", "R", "ky", "kx"]
        args = [kw.get(nm, v) for nm, v in zip(names, good)]
        refused(lambda: lib.cine_grappa_gram(*args, stream()), want, k, f"cine_grappa_gram {what}")

    span = (ky - 1) * R + 1
    bad(EINVAL, "hc < span", hc=span - 1)
    bad(EINVAL, "w < kx", w=kx - 1)
    bad(EUNSUPPORTED, "33 coils", c=33)
    bad(EINVAL, "ky = 3", ky=3)
    bad(EINVAL, "kx = 4", kx=4)
    bad(EINVAL, "R = 1", R=1)
    bad(EINVAL, "R = 9", R=9)
    bad(EWORKSPACE, "a short workspace", ws_bytes=hc * w * c * 16 - 1)
    for nm in ("cal", "gram", "ws"):
        bad(EINVAL, f"null {nm}", **{nm: None})
    bad(EINVAL, "gram off its alignment", gram=out.ptr() + 8)
    for args in ((c, span - 1, w, R, ky, kx), (c, hc, kx - 1, R, ky, kx), (33, hc, w, R, ky, kx), (c, hc, w, R, 3, kx), (c, hc, w, R, ky, 4),
                 (c, hc, w, 1, ky, kx), (c, hc, w, 9, ky, kx)):
        assert lib.cine_grappa_gram_ws_bytes(*args) == 0
    assert lib.cine_grappa_gram(*good, stream()) == 0                              # and the call works after every refusal
    k.finish("cine_grappa_gram after the refusals")


# ================================================================== weights
# (t, c, h, w, R, ky, kx): the three phantom shapes of the CPU test and two wide ones
WEIGHT_SHAPES = [(6, 8, 48, 40, 3, 2, 5), (8, 8, 48, 40, 4, 2, 5), (5, 6, 30, 22, 2, 2, 3), (3, 17, 32, 24, 3, 4, 5), (8, 32, 32, 24, 8, 2, 3)]
_GRAMS = {}


def phantom_gram(shape):
    """The reference's Gram matrix of the TGRAPPA calibration array (all rows) of the noisy phantom; computed once per shape."""
    if shape not in _GRAMS:
        t, c, h, w, R, ky, kx = shape
        _, mask, mk = ref.phantom_slice(t, c, h, w, R)
        cal = ref.calibration_data(mk, mask, "tgrappa", None, h)
        G = ref.gram(cal, R, ky, kx)
        G.setflags(write=False)
        _GRAMS[shape] = G
    return _GRAMS[shape]


def call_weights(k, G, c, R, ky, kx, lam, off=0):
    g = ref.geom(c, R, ky, kx)
    need = L().cine_grappa_weights_ws_bytes(c, R, ky, kx)
    assert need > 0
    d_g = k.raw(torch.from_numpy(np.array(G, dtype=np.complex128)))
    wts = k.out((R - 1, g["ns"], c, 2))
    info = k.out64(4)
    ws = k.ws(need)
    code = L().cine_grappa_weights(d_g.data_ptr(), wts.ptr(), info.ptr(), ws.ptr(), ws.nbytes, c, R, ky, kx, float(lam), stream())
    return code, wts, info


@pytest.mark.parametrize("lam", [1e-4, 1e-2])
@pytest.mark.parametrize("shape", WEIGHT_SHAPES, ids=lambda s: "t%d-c%d-%dx%d-R%d-k%dx%d" % s)
def test_weights_against_numpy_solve(dev, shape, lam):
    t, c, h, w, R, ky, kx = shape
    G = phantom_gram(shape)
    W_ref, info_ref = ref.weights(G, c, R, ky, kx, lam)

    def body(k):
        code, wts, info = call_weights(k, G, c, R, ky, kx, lam)
        assert code == 0, L().cine_last_error()
        return [wts.t, info.t]

    wts, info = twice(dev, 0, body, "cine_grappa_weights")                          # the same bits twice
    W = cplx(wts)
    info = info.numpy()
    err, peak = float(np.abs(W - W_ref).max()), float(np.abs(W_ref).max())
    print(f"lam {lam:g}: ns {ky * kx * c}, max |dW| / max |W| = {err / peak:.3e} (bar {8 * 2.0 ** -24:.3e}), info {info.tolist()}, reference "
          f"{info_ref.tolist()}")
    assert err <= 8 * 2.0 ** -24 * peak
    assert 0 <= info[0] <= 1e-8
    assert abs(info[1] - info_ref[1]) <= 1e-12 * info_ref[1] and abs(info[3] - info_ref[3]) <= 1e-12 * info_ref[3]
    assert abs(info[2] - info_ref[2]) <= 1e-6


def test_weights_of_the_zero_gram_are_exactly_zero(dev):
    c, R, ky, kx = 3, 3, 2, 5
    n = ref.geom(c, R, ky, kx)["n_aug"]
    k = Call(dev, 0)
    code, wts, info = call_weights(k, np.zeros((n, n), np.complex128), c, R, ky, kx, 1e-4)
    assert code == 0, L().cine_last_error()
    k.finish("cine_grappa_weights")
    assert same_bits(wts.t.cpu(), torch.zeros(R - 1, ky * kx * c, c, 2))
    assert info.t.cpu().tolist() == [0.0, 0.0, 0.0, 0.0]


def test_weights_of_a_nan_gram_report_it(dev):
    shape = WEIGHT_SHAPES[2]
    _, c, _, _, R, ky, kx = shape
    G = phantom_gram(shape).copy()
    G[1, 1] = np.nan
    k = Call(dev, 0)
    code, wts, info = call_weights(k, G, c, R, ky, kx, 1e-4)
    assert code == 0, L().cine_last_error()
    k.ins.clear()                                                                    # a NaN never compares equal: the guards are what counts
    k.finish("cine_grappa_weights")
    assert np.isnan(info.t.cpu().numpy()[0])


def test_weights_refusals(dev):
    c, R, ky, kx = 3, 3, 2, 5
    g = ref.geom(c, R, ky, kx)
    lib = L()
    k = Call(dev, 0)
    d_g = k.raw(torch.zeros(g["n_aug"], g["n_aug"], dtype=torch.complex128))
    wts = k.out((R - 1, g["ns"], c, 2))
    info = k.out64(4)
    need = lib.cine_grappa_weights_ws_bytes(c, R, ky, kx)
    ws = k.ws(need)
    good = [d_g.data_ptr(), wts.ptr(), info.ptr(), ws.ptr(), need, c, R, ky, kx, 1e-4]

    def bad(want, what, **kw):
        names = ["gram", "weights", "info", "ws", "ws_bytes", "c", "R", "ky", "kx", "lam"]
        args = [kw.get(nm, v) for nm, v in zip(names, good)]
        refused(lambda: lib.cine_grappa_weights(*args, stream()), want, k, f"cine_grappa_weights {what}")

    bad(EINVAL, "lam = 0", lam=0.0)
    bad(EINVAL, "lam < 0", lam=-1e-4)
    bad(EINVAL, "lam = NaN", lam=float("nan"))
    bad(EINVAL, "lam = inf", lam=float("inf"))
    bad(EUNSUPPORTED, "33 coils", c=33)
    bad(EINVAL, "ky = 3", ky=3)
    bad(EINVAL, "kx = 4", kx=4)
    bad(EINVAL, "R = 1", R=1)
    bad(EINVAL, "R = 9", R=9)
    bad(EWORKSPACE, "a short workspace", ws_bytes=need - 1)
    for nm in ("gram", "weights", "info", "ws"):
        bad(EINVAL, f"null {nm}", **{nm: None})
    bad(EINVAL, "ws off its alignment", ws=ws.ptr() + 8)
    for args in ((33, R, ky, kx), (c, 1, ky, kx), (c, 9, ky, kx), (c, R, 3, kx), (c, R, ky, 4)):
        assert lib.cine_grappa_weights_ws_bytes(*args) == 0
    assert lib.cine_grappa_weights_ws_bytes(32, 8, 4, 7) > 0                        # n_aug = 1120, the largest there is


# ================================================================== apply
def apply_cases():
    axes = {"c": [1, 3, 8, 17, 32], "R": [2, 3, 5, 8], "kernel": [0, 1, 2, 3], "t": [1, 3], "h": ["R+1", "13", "48"], "w": [1, 5, 33, 67, 130]}
    out = []
    for case in sweep(20252, axes, 48):
        ky, kx = KERNELS[case["kernel"]]
        h = {"R+1": case["R"] + 1, "13": 13, "48": 48}[case["h"]]
        out.append({"c": case["c"], "R": case["R"], "ky": ky, "kx": kx, "t": case["t"], "h": h, "w": case["w"]})
    return out


def apply_inputs(case):
    """(k-space with NaN in every row that is not acquired, mask, offsets, weights): frame f lies on the lattice of residue (f + seed)
    mod R; with three frames the middle one loses a lattice row (offset -1) and the last carries an ACS block inside the lattice."""
    c, R, ky, kx, t, h, w = (case[x] for x in ("c", "R", "ky", "kx", "t", "h", "w"))
    seed = hash_case(case)
    rs = np.random.RandomState(seed)
    offs = [(f + seed) % R for f in range(t)]
    mask = ref.lattice_mask(t, h, R, offsets=offs)
    if t == 3:
        mask[1, np.flatnonzero(mask[1])[0]] = 0
        n_acs = min(h // 3, 8)
        mask[2, h // 2 - n_acs // 2:h // 2 - n_acs // 2 + n_acs] = 1
    off, _ = ref.offsets(mask, R)
    k = (rs.standard_normal((t, c, h, w)) + 1j * rs.standard_normal((t, c, h, w))).astype(np.complex64)
    k = np.where(mask.astype(bool)[:, None, :, None], k, np.complex64(complex(np.nan, np.nan)))
    ns = ky * kx * c
    W = ((rs.standard_normal((R - 1, ns, c)) + 1j * rs.standard_normal((R - 1, ns, c))) / np.sqrt(ns)).astype(np.complex64)
    return k, mask, off, W


@pytest.mark.parametrize("case", apply_cases(), ids=case_id)
def test_apply_against_float64(dev, case):
    c, R, ky, kx, t, h, w = (case[x] for x in ("c", "R", "ky", "kx", "t", "h", "w"))
    ksp, mask, off, W = apply_inputs(case)
    if t == 3 and h > R + 1:
        assert off[1] == -1
    want, mag = ref.apply(ksp, W, mask, off, R, ky, kx, bound=True)
    x_in, w_in = pairs(ksp), pairs(W)
    d_mask, d_off = torch.from_numpy(mask), torch.from_numpy(off.astype(np.int32))

    def out_of_place(k):
        d_k, d_w = k.inp_among_nan(x_in), k.inp(w_in)
        out = k.out((t, c, h, w, 2))
        code = L().cine_grappa_apply(d_k.data_ptr(), d_w.data_ptr(), k.raw(d_mask).data_ptr(), k.raw(d_off).data_ptr(), out.ptr(), t, c, h, w, R,
                                     ky, kx, stream())
        assert code == 0, L().cine_last_error()
        return [out.t]

    def in_place(k):
        d_w = k.inp(w_in)
        buf = k.out((t, c, h, w, 2), fill=x_in)
        code = L().cine_grappa_apply(buf.ptr(), d_w.data_ptr(), k.raw(d_mask).data_ptr(), k.raw(d_off).data_ptr(), buf.ptr(), t, c, h, w, R, ky,
                                     kx, stream())
        assert code == 0, L().cine_last_error()
        return [buf.t]

    got = at_offsets(dev, (0, 2), out_of_place, "cine_grappa_apply")[0]             # twice at both placements, guards intact, the same bits
    same = at_offsets(dev, (0, 2), in_place, "cine_grappa_apply in place")[0]
    assert same_bits(got, same), "in place gives other bits than out of place"

    acquired = torch.from_numpy(mask.astype(bool))
    kept = acquired.clone()
    kept[torch.from_numpy(off < 0)] = True                                           # frames without a lattice are left alone
    sel = kept[:, None, :, None, None].expand(t, c, h, w, 2)
    assert torch.equal(got.view(torch.int32)[sel], x_in.view(torch.int32)[sel]), "a row that is not a target changed"
    target = ~kept.numpy()
    G = cplx(got)
    tg = np.broadcast_to(target[:, None, :, None], G.shape)
    assert not np.isnan(G[tg].real).any() and not np.isnan(G[tg].imag).any(), "a target was not written, or a row that is no source was read"
    bar = (2 * ky * kx * c + 1) * 2.0 ** -24
    e_re, e_im = np.abs(G.real - want.real)[tg], np.abs(G.imag - want.imag)[tg]
    b_re, b_im = bar * mag.real[tg], bar * mag.imag[tg]
    if tg.any():
        worst = max(float((e_re / np.maximum(b_re, 1e-300)).max()), float((e_im / np.maximum(b_im, 1e-300)).max()))
        print(f"{case_id(case)}: {int(target.sum())} target rows, worst error {worst:.3f} of its bound")
    assert (e_re <= b_re).all() and (e_im <= b_im).all()


def test_apply_refusals(dev):
    c, R, ky, kx, t, h, w = 3, 3, 2, 5, 2, 13, 9
    ns = ky * kx * c
    lib = L()
    k = Call(dev, 0)
    d_k = k.inp(torch.ones(2 * t, c, h, w, 2))[:t]                                   # room behind the k-space for the overlap cases
    d_w = k.inp(torch.ones(R - 1, ns, c, 2))
    d_mask = k.raw(torch.from_numpy(ref.lattice_mask(t, h, R)))
    d_off = k.raw(torch.tensor([0, 1], dtype=torch.int32))
    out = k.out((t, c, h, w, 2))
    good = [d_k.data_ptr(), d_w.data_ptr(), d_mask.data_ptr(), d_off.data_ptr(), out.ptr(), t, c, h, w, R, ky, kx]
    names = ["in", "weights", "mask", "offsets", "out", "t", "c", "h", "w", "R", "ky", "kx"]

    def bad(want, what, **kw):
        args = [kw.get(nm, v) for nm, v in zip(names, good)]
        refused(lambda: lib.cine_grappa_apply(*args, stream()), want, k, f"cine_grappa_apply {what}")

    for nm in names[:5]:
        bad(EINVAL, f"null {nm}", **{nm: None})
    bad(EINVAL, "t = 0", t=0)
    bad(EINVAL, "w = 0", w=0)
    bad(EUNSUPPORTED, "33 coils", c=33)
    bad(EINVAL, "ky = 3", ky=3)
    bad(EINVAL, "kx = 4", kx=4)
    bad(EINVAL, "R = 1", R=1)
    bad(EINVAL, "R = 9", R=9)
    bad(EINVAL, "in off its alignment", **{"in": d_k.data_ptr() + 4})
    bad(EINVAL, "out off its alignment", out=out.ptr() + 4)
    bad(EINVAL, "out overlaps in", out=d_k.data_ptr() + 8)
    bad(EINVAL, "out ends inside in", out=d_k.data_ptr() + 8 * c * h * w)
    bad(EUNSUPPORTED, "too many frames", t=65536)
    assert lib.cine_grappa_apply(*good, stream()) == 0                               # and the call works after every refusal
    k.finish("cine_grappa_apply after the refusals")
