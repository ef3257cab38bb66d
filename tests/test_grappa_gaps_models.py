"""cine_hip.grappa with ``accel=None`` on the GPU: ``grappa`` end to end on an equispaced-style slice against the float64 reference
(tests/grappa_gaps_reference.py) within the model-level bar of tests/test_grappa_models.py, max |delta| / peak <= 1e-4; ``max_unfilled``;
``Grappa(accel=None, gaps=...)`` captured into a graph and through ``SlicePipeline`` bit for bit against the eager calls; and an integer
``accel`` still on the lattice path, bit for bit against the composition of its entry points."""
import numpy as np
import pytest
import torch

import grappa_gaps_reference as gref
import grappa_reference as ref

pytestmark = pytest.mark.gpu

MODEL_BAR = 1e-4
T, C, H, W, KERNEL, ACS = 4, 8, 48, 40, (2, 5), (19, 29)


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "-m gpu tests need an MI355X"
    return torch.device("cuda:0")


def pairs(z):
    return torch.from_numpy(np.stack((z.real, z.imag), -1).astype(np.float32))


def uneven_mask(t, h, step, acs, start=0):
    """Equispaced in the manner of the reference: frame f acquires the rows round(f + start + step j) -- steps floor(step) and
    ceil(step) -- and the centre block."""
    m = np.zeros((t, h), np.uint8)
    for f in range(t):
        m[f, np.around(np.arange((f + start) % int(step), h - 1, step)).astype(int)] = 1
    m[:, acs[0]:acs[1]] = 1
    return m


def problem(dev, mask=None, scale=1.0):
    """(masked k-space (1, t, c, h, w, 2), mask (1, t, 1, h, 1, 1)) on the device, and the numpy pair."""
    full = ref.phantom_slice(T, C, H, W, 2)[0]
    mask = uneven_mask(T, H, 3.4, ACS) if mask is None else mask
    mk = (scale * full * mask[:, None, :, None]).astype(np.complex64)
    return pairs(mk)[None].to(dev), torch.from_numpy(mask.reshape(1, T, 1, H, 1, 1)).to(dev), mk, mask


def test_grappa_gaps_against_the_reference(dev):
    from cine_hip import grappa as G
    d_mk, d_mask, mk, mask = problem(dev)
    want, info_ref, sizes_ref, unfilled_ref = gref.grappa(mk, mask, KERNEL[1], 1e-4, acs=ACS)
    assert {3, 4} <= set(sizes_ref) and not unfilled_ref.any()
    with pytest.raises(ValueError, match="no lattice"):                               # what the lattice path makes of this mask
        G.grappa(d_mk, d_mask, 3, kernel=KERNEL, acs=ACS)
    filled, info, sizes, unfilled = G.grappa(d_mk, d_mask, kernel=KERNEL, lam=1e-4, acs=ACS, output="kspace", record=True)
    assert sizes == sizes_ref and tuple(info.shape) == (1, len(sizes), 4) and unfilled.cpu().tolist() == [unfilled_ref.tolist()]
    assert tuple(filled.shape) == (1, T, C, H, W, 2)
    got = filled[0].cpu().numpy().astype(np.float64)
    got = got[..., 0] + 1j * got[..., 1]
    e_k = float(np.abs(got - want).max() / np.abs(want).max())
    acq = mask.astype(bool).nonzero()
    assert (got[acq[0], :, acq[1]] == mk[acq[0], :, acq[1]]).all()
    img = G.grappa(d_mk, d_mask, kernel=KERNEL, lam=1e-4, acs=ACS)
    rss = ref.rss(want)
    e_i = float(np.abs(img[0].cpu().numpy() - rss).max() / rss.max())
    fits = {s: (float(info[0, i, 2]), float(info_ref[s][2])) for i, s in enumerate(sizes)}
    print(f"steps {sizes}: k-space {e_k:.3e}, RSS image {e_i:.3e} of the peak (bar {MODEL_BAR:g}); fit per step (device, reference) {fits}")
    assert e_k <= MODEL_BAR and e_i <= MODEL_BAR
    assert float(info[0, :, 0].max()) <= G.RESIDUAL_MAX
    explicit = G.grappa(d_mk, d_mask, None, KERNEL, 1e-4, acs=ACS, output="kspace", gaps=sizes)
    assert torch.equal(explicit, filled)                                              # "auto" is the steps that occur
    mod = G.Grappa(accel=None, gaps=sizes, kernel=KERNEL, lam=1e-4, acs=ACS).eval()
    assert torch.equal(mod(d_mk, d_mask), img) and torch.equal(mod(d_mk, d_mask, output="kspace"), filled)
    assert mod.last_info["unfilled"].cpu().tolist() == [[0] * T] and tuple(mod.last_info["info"].shape) == (1, len(sizes), 4)
    plan = G.plan_gaps(mask)[0]
    assert mod.last_info["count"].cpu().tolist() == [[len(g) for g in plan]]
    table, count, _ = G.gap_table(d_mask, sizes)
    assert tuple(table.shape) == (1, T, H // 2 + 1, 2)
    for f in range(T):
        assert table[0, f, :int(count[0, f])].cpu().tolist() == [list(g) for g in plan[f]]


def test_max_unfilled(dev):
    from cine_hip import grappa as G
    mask = uneven_mask(T, H, 3.4, ACS)
    mask[2, 30:38] = 0                                                                # frame 2: rows 29 and 38 are nine apart
    mask[2, 38] = 1
    d_mk, d_mask, mk, _ = problem(dev, mask)
    missing, left = int((mask == 0).sum()), 8
    with pytest.raises(ValueError, match="row 30 of frame 2"):
        G.grappa(d_mk, d_mask, kernel=KERNEL, acs=ACS)
    with pytest.raises(ValueError, match="unfilled"):
        G.grappa(d_mk, d_mask, kernel=KERNEL, acs=ACS, max_unfilled=(left - 0.5) / missing)
    filled, _, sizes, unfilled = G.grappa(d_mk, d_mask, kernel=KERNEL, acs=ACS, max_unfilled=left / missing, output="kspace", record=True)
    assert unfilled.cpu().tolist() == [[0, 0, left, 0]]
    assert not filled[0, 2, :, 30:38].any() and bool(filled[0, 2, :, 40].any())       # the rows of the gap of nine stay zero, the next gap is filled
    want = gref.grappa(mk, mask, KERNEL[1], 1e-4, acs=ACS)[0]
    got = filled[0].cpu().numpy().astype(np.float64)
    assert float(np.abs(got[..., 0] + 1j * got[..., 1] - want).max() / np.abs(want).max()) <= MODEL_BAR
    with pytest.raises(ValueError, match="row 1 of frame 0"):                         # a step that occurs but has no kernels
        G.grappa(d_mk, d_mask, kernel=KERNEL, acs=ACS, gaps=(2, 4), max_unfilled=left / missing)
    with pytest.raises(ValueError, match="acquired by no frame"):
        G.grappa(d_mk, d_mask, kernel=KERNEL, acs=(ACS[0], 34), max_unfilled=1.0)
    with pytest.raises(ValueError, match="calibration block of 4 rows"):              # steps up to 4 need five rows
        G.grappa(d_mk, d_mask, kernel=KERNEL, acs=(20, 24), max_unfilled=1.0)


def test_grappa_gaps_is_capturable(dev):
    """Captured and replayed twice: the eager bits.  The process keeps its default number of hardware queues."""
    from cine_hip import grappa as G
    from cine_hip.pipeline import pipeline_streams
    d_mk, d_mask, _, _ = problem(dev)
    model = G.Grappa(accel=None, gaps=(2, 3, 4, 5), kernel=KERNEL, acs=ACS).eval()    # step 5 does not occur: its kernels are fitted and idle
    want = model(d_mk, d_mask).clone()
    assert torch.equal(want, G.grappa(d_mk, d_mask, kernel=KERNEL, acs=ACS))
    s = pipeline_streams(dev, 1)[0][0]                                                # a stream of the pipelines' pool: the test creates none of its own
    with torch.cuda.stream(s):
        warm = model(d_mk, d_mask).clone()
    s.synchronize()
    assert torch.equal(warm, want)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=s):
        out = model(d_mk, d_mask)
    for _ in range(2):
        out.fill_(float("nan"))
        g.replay()
        torch.cuda.synchronize()
        assert torch.equal(out, want)
    assert model.last_info["unfilled"].cpu().tolist() == [[0] * T] and float(model.last_info["info"][0, :, 0].max()) <= G.RESIDUAL_MAX


def test_pipeline_submit(dev):
    from cine_hip import grappa as G
    from cine_hip.pipeline import SlicePipeline
    model = G.Grappa(accel=None, gaps=(2, 3, 4), kernel=KERNEL, acs=ACS).eval()
    ins = []
    for j in range(3):                                                                # three slices whose frames start at other rows
        d_mk, d_mask, _, _ = problem(dev, uneven_mask(T, H, 3.4, ACS, start=j), scale=1.0 + 0.25 * j)
        ins.append((d_mk, d_mask))
    want = [model(*a).clone() for a in ins]
    assert not torch.equal(want[0], want[1]) and all(bool(torch.isfinite(v).all()) for v in want)
    with SlicePipeline(model, slots=2) as pipe:
        assert pipe.graphs
        for j, a in enumerate(ins):
            pipe.submit(*a, tag=j)
        got = dict(pipe.drain())
        assert pipe.set_builds == 1
    for j in range(3):
        assert torch.equal(got[j], want[j]), j


def test_an_integer_accel_still_takes_the_lattice_path(dev):
    from cine_hip import grappa as G
    t, c, h, w, R = 6, 8, 48, 40, 3
    _, mask, mk = ref.phantom_slice(t, c, h, w, R)
    d_mk, d_mask = pairs(mk)[None].to(dev), torch.from_numpy(mask.reshape(1, t, 1, h, 1, 1)).to(dev)
    filled, info, off = G.grappa(d_mk, d_mask, R, kernel=KERNEL, output="kspace", record=True)
    offsets, status = G.lattice_offsets(d_mask, R)
    cal = G.calibration_data(d_mk, d_mask)
    weights, winfo = G.grappa_weights(cal[0], R, KERNEL, 1e-4)
    want = G.grappa_apply(d_mk[0], weights, d_mask.view(t, h), offsets[0], R, KERNEL)
    assert torch.equal(filled[0], want) and torch.equal(info[0], winfo) and torch.equal(off, offsets) and not status.any()
    mod = G.Grappa(accel=R, kernel=KERNEL).eval()
    assert torch.equal(mod(d_mk, d_mask, output="kspace"), filled) and set(mod.last_info) == {"info", "offsets", "status"}
    # and the gap path on the same lattice: the lattice kernels of step R from the same calibration, the bits of the lattice path
    gapped, ginfo, sizes, unfilled = G.grappa(d_mk, d_mask, kernel=KERNEL, output="kspace", record=True)
    assert sizes == (R,) and not unfilled.any() and torch.equal(ginfo[0, 0], winfo) and torch.equal(gapped, filled)
