"""SlicePipeline on the GPU: every output equals the eager forward of the same slice bit for bit.

N = 2S + 1 slices with different seeds and different centre widths, so that masks and ACS windows differ between slices
and every buffer set / graph is replayed for more than one slice."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu


def _dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


def _model(name):
    import reconstruction.models as M
    if name == "cfg2":
        return M.VarNet(6, 8, 3, 16, 3, "XF"), 1, ("lambda",)
    if name == "xpdnet_xt":
        return M.XPDNet(num_cascades=2, sens_chans=4, sens_pools=2, n_scales=2, n_filters_per_scale=[8, 16], n_convs_per_scale=[1, 1],
                        first_conv_n_filters=8, n_primal=2, dynamic_type="XT"), 6, ()
    if name == "cinenet_3d":
        return M.CineNet(2, 3, 4, 2, "3D"), 7, ("lambda",)
    return M.VarNet_RNN(2, 4, 2, 6), 9, ("lambda",)


SHAPES = {"cfg2": (15, 15, 200, 200, 4, 0.0), "xpdnet_xt": (5, 3, 24, 20, 4, 0.01), "cinenet_3d": (5, 3, 24, 20, 4, 0.0),
          "varnet_rnn": (5, 3, 24, 20, 4, 0.0)}
NEEDS_SENS = {"cinenet_3d"}
N = 7                                                   # 2 S + 1 for S = 3 (S = 1 uses the first 3)


def _slices(name, n, shape=None, seed0=100):
    from cine_hip import synth
    t, c, h, w, accel, noise = shape or SHAPES[name]
    centre = (lambda j: 10 + 2 * (j % 3)) if h >= 100 else (lambda j: 2 + j % 3)        # (h / accel lines in all)
    return [synth.make_cine_slice(t, c, h, w, accel=accel, center_lines=centre(j), seed=seed0 + j, noise_std=noise) for j in range(n)]


class Case:
    def __init__(self, name):
        from cine_hip import ops, synth
        dev = _dev()
        net, wseed, keep = _model(name)
        synth.fill_parameters_(net, wseed, keep=keep)
        self.name, self.net, self.dev = name, net.to(dev).eval(), dev
        self.exs = _slices(name, N)
        self.sens = name in NEEDS_SENS
        self.want, self.zf = [], []
        wins = set()
        for ex in self.exs:
            mk, mask = ex["masked_kspace"].to(dev), ex["mask"].to(dev)
            args = (mk, mask, ex["sens_maps"].to(dev)) if self.sens else (mk, mask)
            self.want.append(self.net(*args).clone())          # the eager forward on the current stream
            self.zf.append(ops.zero_filled_rss(mk))
            wins.add(tuple(ops.acs_window_dev(mask).cpu().tolist()))
        torch.cuda.synchronize()
        assert len(wins) >= 3, wins                              # the slices' ACS windows differ: a replay must follow its slice's mask

    def inputs(self, j, form):
        ex = self.exs[j]
        mk, mask, sens = ex["masked_kspace"], ex["mask"], ex["sens_maps"] if self.sens else None
        if form == "device":
            return mk.to(self.dev), mask.to(self.dev), None if sens is None else sens.to(self.dev)
        if form == "pinned":
            return mk.pin_memory(), mask.pin_memory(), None if sens is None else sens.pin_memory()
        as_c = lambda x: np.ascontiguousarray(torch.view_as_complex(x).numpy())           # complex64 (b, t, c, h, w) numpy
        return as_c(mk), mask.numpy().astype(np.float32), None if sens is None else as_c(sens)


_CASES = {}


@pytest.fixture
def case(request):
    name = request.param
    if name not in _CASES:
        _CASES.clear()                                           # one model family's slices and references at a time
        _CASES[name] = Case(name)
    return _CASES[name]


def _run(case, S, form="device", n=None, **kw):
    from cine_hip.pipeline import SlicePipeline
    n = n or 2 * S + 1
    got, order = {}, []
    with SlicePipeline(case.net, slots=S, **kw) as pipe:
        for j in range(n):
            mk, mask, sens = case.inputs(j, form)
            h = pipe.submit(mk, mask, sens, tag=f"s{j}")
            assert (h.index, h.slot) == (j, j % S) and h.parity == (j // S) & 1
            for tag, out in pipe.results():
                order.append(tag); got[tag] = out
        for tag, out in pipe.drain():
            order.append(tag); got[tag] = out
        assert pipe.pending() == 0
    assert order == [f"s{j}" for j in range(n)]
    return [got[f"s{j}"] for j in range(n)]


def _same(a, b):
    return a.shape == b.shape and torch.equal(a.cpu(), b.cpu())


@pytest.mark.parametrize("form", ["device", "pinned", "numpy"])
@pytest.mark.parametrize("S", [1, 3])
@pytest.mark.parametrize("case", ["cfg2", "xpdnet_xt", "cinenet_3d", "varnet_rnn"], indirect=True)     # (innermost: one model at a time)
def test_pipeline_matches_eager_bit_for_bit(case, S, form):
    outs = _run(case, S, form)
    for j, o in enumerate(outs):
        assert o.is_cuda and o.device == case.dev
        assert _same(o, case.want[j]), (case.name, S, form, j, float((o - case.want[j]).abs().max()))


@pytest.mark.parametrize("case", ["cfg2", "cinenet_3d"], indirect=True)
def test_host_outputs_and_zero_filled(case):
    outs = _run(case, 3, "pinned", out="host", zero_filled=True)
    for j, (o, z) in enumerate(outs):
        assert not o.is_cuda and o.is_pinned() and not z.is_cuda
        assert _same(o, case.want[j]), j
        assert _same(z, case.zf[j]), j


@pytest.mark.parametrize("S", [1, 3])
@pytest.mark.parametrize("case", ["cfg2", "varnet_rnn"], indirect=True)
def test_eager_mode_gives_the_same_bits(case, S):
    outs = _run(case, S, "device", graphs=False, zero_filled=True)
    for j, (o, z) in enumerate(outs):
        assert _same(o, case.want[j]), j
        assert _same(z, case.zf[j]), j


@pytest.mark.parametrize("case", ["xpdnet_xt"], indirect=True)
def test_shape_change_midstream(case):
    from cine_hip.pipeline import SlicePipeline
    other = _slices("xpdnet_xt", 4, shape=(5, 4, 32, 24, 4, 0.01), seed0=300)
    dev = case.dev
    want_b = [case.net(ex["masked_kspace"].to(dev), ex["mask"].to(dev)).clone() for ex in other]
    plan = [("a", 0), ("a", 1), ("b", 0), ("b", 1), ("b", 2), ("a", 2), ("a", 3), ("b", 3), ("a", 4)]
    got = []
    with SlicePipeline(case.net, slots=2) as pipe:
        for which, j in plan:
            ex = case.exs[j] if which == "a" else other[j]
            pipe.submit(ex["masked_kspace"].pin_memory(), ex["mask"], tag=(which, j))
        got = list(pipe.drain())
    assert [t for t, _ in got] == plan
    for (which, j), o in got:
        assert _same(o, case.want[j] if which == "a" else want_b[j]), (which, j)


@pytest.mark.parametrize("case", ["varnet_rnn"], indirect=True)
def test_pipeline_creates_no_side_streams_and_rejects_after_close(case):
    from cine_hip import ops
    from cine_hip._lib import CineHipError
    from cine_hip.pipeline import SlicePipeline
    pipe = SlicePipeline(case.net, slots=3)
    mk, mask, _ = case.inputs(0, "device")
    for j in range(4):
        pipe.submit(*case.inputs(j, "device")[:2])
    ids = {s.cuda_stream for s in pipe.streams + [pipe.copy_stream]}
    assert not [k for k in ops._SIDE_STREAMS if k[1] in ids]
    got = [o for _, o in pipe.drain()]
    assert all(_same(o, case.want[j]) for j, o in enumerate(got))
    with pytest.raises(CineHipError):
        pipe.submit(mk, mask[..., :3, :, :])                  # a mask that does not fit the k-space
    pipe.close()
    with pytest.raises(CineHipError):
        pipe.submit(mk, mask)
