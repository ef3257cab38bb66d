"""cine_hip.selfsup on the host: the Omega -> (Theta, Lambda) split, and the loss formula restated in float64 torch on the oracle's
sens_expand against a case computed by hand."""
import math

import numpy as np
import pytest
import torch

from cine_hip.selfsup import split_mask


def omega(layout, t, seed=3, b=2, h=24, w=20):
    g = torch.Generator().manual_seed(seed)
    ww = 1 if layout == "row" else w
    m = (torch.rand(b, t, 1, h, ww, 1, generator=g) < 0.45).to(torch.uint8)
    if layout == "row":
        m[:, :, :, h // 2 - 3:h // 2 + 3] = 1
    else:
        m[:, :, :, h // 2 - 3:h // 2 + 3, w // 2 - 3:w // 2 + 3] = 1
    return m


def centre(layout, h, w, acs):
    c = torch.zeros(h, 1 if layout == "row" else w, dtype=torch.bool)
    if layout == "row":
        c[h // 2 - acs // 2:h // 2 - acs // 2 + acs] = True
    else:
        c[h // 2 - acs // 2:h // 2 - acs // 2 + acs, w // 2 - acs // 2:w // 2 - acs // 2 + acs] = True
    return c


@pytest.mark.parametrize("t", [1, 3])
@pytest.mark.parametrize("layout", ["row", "plane"])
def test_split_mask(layout, t):
    rho, acs = 0.4, 4
    m = omega(layout, t)
    keep = m.clone()
    theta, lam = split_mask(m, rho=rho, acs=acs, rng=np.random.default_rng(11))
    assert torch.equal(m, keep), "the input was modified"
    assert theta.dtype == lam.dtype == torch.uint8 and theta.shape == lam.shape == m.shape
    assert int((theta & lam).sum()) == 0, "Theta and Lambda overlap"
    assert torch.equal(theta | lam, m), "Theta + Lambda is not Omega"
    b, _, _, h, w, _ = m.shape
    c = centre(layout, h, 20, acs)
    for ib in range(b):
        for it in range(t):
            fr, th, la = (x[ib, it, 0, :, :, 0].bool() for x in (m, theta, lam))
            assert bool(fr[c].all()) and bool(th[c].all()) and not bool(la[c].any()), "the ACS region is not entirely in Theta"
            n = int((fr & ~c).sum())
            assert int(la.sum()) == int(round(rho * n)) > 0, (ib, it)
    theta2, lam2 = split_mask(m, rho=rho, acs=acs, rng=np.random.default_rng(11))
    assert torch.equal(theta, theta2) and torch.equal(lam, lam2), "the same seed gives another split"
    _, lam3 = split_mask(m, rho=rho, acs=acs, rng=np.random.default_rng(12))
    assert not torch.equal(lam, lam3), "another seed gives the same split"
    theta0, lam0 = split_mask(m, rho=0.0, acs=acs, rng=np.random.default_rng(11))
    assert int(lam0.sum()) == 0 and torch.equal(theta0, m)


def test_split_mask_prefers_the_centre_and_checks_its_arguments():
    m = torch.ones(1, 1, 1, 64, 1, 1, dtype=torch.uint8)
    counts = torch.zeros(64)
    rng = np.random.default_rng(5)
    for _ in range(200):
        counts += split_mask(m, rho=0.25, rng=rng)[1].reshape(-1).float()
    assert counts[24:40].sum() > 2 * (counts[:8].sum() + counts[56:].sum())             # a Gaussian of std 16 rows around row 32
    with pytest.raises(ValueError):
        split_mask(m, rho=1.5)
    with pytest.raises(ValueError):
        split_mask(torch.ones(4, 4))


def loss_formula(u, y, lam):
    r, v = lam * (u - y), lam * y
    return 0.5 * (r * r).sum().sqrt() / (v * v).sum().sqrt() + 0.5 * r.abs().sum() / v.abs().sum()


def test_the_loss_formula_on_a_case_computed_by_hand():
    """1 x 1 x 1 x 2 x 3: the image is a unit impulse at the centre (row 1, column 1) and the map is the constant 2 + i, so the centered
    ortho FFT of S x is (2 + i) / sqrt(6) at every point.  With y = 1 - i everywhere and Lambda = {(0, 0), (1, 2)}:
    r = (2 / sqrt 6 - 1) + (1 / sqrt 6 + 1) i at both points."""
    from oracle import varnet_ref as V
    x = torch.zeros(1, 1, 1, 2, 3, 2, dtype=torch.float64)
    x[0, 0, 0, 1, 1, 0] = 1.0
    s = torch.zeros(1, 1, 1, 2, 3, 2, dtype=torch.float64)
    s[..., 0], s[..., 1] = 2.0, 1.0
    u = V.VarNetBlock.sens_expand(x, s)
    q = 1 / math.sqrt(6)
    assert torch.allclose(u[..., 0], torch.full((1, 1, 1, 2, 3), 2 * q, dtype=torch.float64), atol=1e-14)
    assert torch.allclose(u[..., 1], torch.full((1, 1, 1, 2, 3), q, dtype=torch.float64), atol=1e-14)
    y = torch.zeros_like(u)
    y[..., 0], y[..., 1] = 1.0, -1.0
    lam = torch.zeros(1, 1, 1, 2, 3, 1, dtype=torch.float64)
    lam[0, 0, 0, 0, 0, 0] = lam[0, 0, 0, 1, 2, 0] = 1.0
    re, im = 2 * q - 1, q + 1
    r2, r1 = 2 * (re * re + im * im), 2 * (abs(re) + abs(im))
    y2, y1 = 2 * 2.0, 2 * 2.0
    want = 0.5 * math.sqrt(r2) / math.sqrt(y2) + 0.5 * r1 / y1
    assert abs(float(loss_formula(u, y, lam)) - want) < 1e-14
    assert math.isnan(float(loss_formula(u, y, torch.zeros_like(lam))))                    # an empty Lambda: 0 / 0


def test_the_models_refuse_an_unknown_output():
    from cine_hip import ops
    assert ops.complex_output("complex") and not ops.complex_output("magnitude")
    with pytest.raises(ValueError):
        ops.complex_output("phase")
