"""cine_gate_readouts through ctypes against float64 (tests/gating_reference.py), the contract of include/cine_hip.h.

row_elems in {1, 3, 21, 485, 960, 3900}: odd and even sizes (the 16-byte and the 8-byte form), shorter than a wave, one chunk with a
ragged end, several chunks (a chunk is 512 accesses: 3900 complex samples are 4 chunks of 16-byte accesses and 8 of 8-byte ones).
rows in {1, 14, 120}; 40 readouts; rows of 0, 1, 2, 3 and 9 entries and one row of 40; indices repeated within and across rows; the last
four readouts are referenced by no row and hold NaN, so a read of them would show.  Every case runs with lines and out on a 16-byte
boundary and 8 bytes past one (where an even row_elems takes the 8-byte form too)."""
import numpy as np
import pytest
import torch

from gating_reference import check_gated
from kernel_sweep import EINVAL, EUNSUPPORTED, GUARD, GUARD_VALUE, L, same_bits, stream

pytestmark = pytest.mark.gpu

N_LINES, N_USED = 40, 36
ROW_ELEMS = [1, 3, 21, 485, 960, 3900]
ROWS = [1, 14, 120]
POPULATIONS = [1, 0, 2, 3, 9]


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "-m gpu tests need an MI355X"
    return torch.device("cuda:0")


def make_csr(rows, seed):
    """A CSR matrix over N_LINES readouts that uses the first N_USED only.  Row populations cycle through POPULATIONS; one row has 40
    entries (with one row only, the seed picks its population from all six).  Every other single-entry row has the weight 1.0."""
    rs = np.random.RandomState(seed)
    pops = [POPULATIONS[r % len(POPULATIONS)] for r in range(rows)]
    if rows == 1:
        pops = [(POPULATIONS + [40])[seed % 6]]
    else:
        pops[rows // 2] = 40
    row_ptr = np.concatenate(([0], np.cumsum(pops))).astype(np.int32)
    index = rs.randint(0, N_USED, size=int(row_ptr[-1])).astype(np.int32)
    weight = rs.uniform(-1.0, 1.0, size=index.shape[0]).astype(np.float32)
    ones = [r for r in range(rows) if pops[r] == 1]
    for r in ones[::2]:
        weight[row_ptr[r]] = 1.0
    return row_ptr, index, weight


def make_lines(row_elems, seed):
    rs = np.random.RandomState(seed)
    x = rs.standard_normal((N_LINES, row_elems, 2)).astype(np.float32)
    x[N_USED:] = np.nan
    return x


def placed(x, off, dev, fill=None):
    """x (numpy float32) on the device at a storage offset of off floats past a 16-byte boundary, between guard floats; (buffer, view)."""
    lo = 4 * ((GUARD + 3) // 4) + off
    buf = torch.full((lo + x.size + GUARD,), GUARD_VALUE, device=dev)
    view = buf[lo:lo + x.size].view(x.shape)
    assert (view.data_ptr() - 4 * off) % 16 == 0
    view.copy_(torch.from_numpy(x)) if fill is None else view.fill_(fill)
    return buf, view


def guards_intact(buf, view):
    lo = (view.data_ptr() - buf.data_ptr()) // 4
    return bool((buf[:lo] == GUARD_VALUE).all()) and bool((buf[lo + view.numel():] == GUARD_VALUE).all())


def csr_dev(row_ptr, index, weight, dev):
    pad = lambda a: np.concatenate((a, np.zeros(1, a.dtype)))               # one spare entry: never a zero-size allocation
    return tuple(torch.from_numpy(pad(a)).to(dev) for a in (row_ptr, index, weight))


def call(lines, out, csr, rows, row_elems, n_lines=N_LINES):
    return L().cine_gate_readouts(lines.data_ptr(), out.data_ptr(), csr[0].data_ptr(), csr[1].data_ptr(), csr[2].data_ptr(), n_lines, rows,
                                  row_elems, stream())


@pytest.mark.parametrize("rows", ROWS)
@pytest.mark.parametrize("row_elems", ROW_ELEMS)
def test_gate_readouts_against_float64(dev, row_elems, rows):
    seed = 31 * row_elems + rows
    row_ptr, index, weight = make_csr(rows, seed)
    lines = make_lines(row_elems, seed + 1)
    csr = csr_dev(row_ptr, index, weight, dev)
    first = None
    for off in (0, 2):                                                        # 16-byte aligned; 8 bytes past: the 8-byte form
        lbuf, ld = placed(lines, off, dev)
        obuf, od = placed(np.empty((rows, row_elems, 2), np.float32), off, dev, fill=float("nan"))
        assert call(ld, od, csr, rows, row_elems) == 0, L().cine_last_error()
        torch.cuda.synchronize()
        got = od.clone()
        assert not bool(torch.isnan(got).any()), "an element of out was not written (or an unreferenced readout was read)"
        assert guards_intact(obuf, od) and guards_intact(lbuf, ld), "wrote outside out"
        assert same_bits(ld.cpu()[:N_USED], torch.from_numpy(lines[:N_USED])), "the readouts were written"
        worst = check_gated(got.cpu().numpy(), lines, row_ptr, index, weight, f"row_elems {row_elems} rows {rows} offset {off}")
        print(f"row_elems {row_elems} rows {rows} offset {off}: worst error {worst:.3f} of its bar")
        od.fill_(float("inf"))                                                # the prior content does not matter; the same bits again
        assert call(ld, od, csr, rows, row_elems) == 0
        torch.cuda.synchronize()
        assert same_bits(od, got), "two calls gave different bits"
        if first is None:
            first = got
        else:
            assert same_bits(got, first), "the 8-byte form gave other bits than the 16-byte form"


def test_gate_readouts_is_capturable(dev):
    rows, row_elems = 14, 485
    row_ptr, index, weight = make_csr(rows, 5)
    lines = make_lines(row_elems, 6)
    csr = csr_dev(row_ptr, index, weight, dev)
    ld = torch.from_numpy(lines).to(dev)
    od = torch.full((rows, row_elems, 2), float("nan"), device=dev)
    assert call(ld, od, csr, rows, row_elems) == 0
    torch.cuda.synchronize()
    want = od.clone()
    s = torch.cuda.Stream(dev)
    g = torch.cuda.CUDAGraph()
    od.fill_(float("nan"))
    torch.cuda.synchronize()
    with torch.cuda.graph(g, stream=s):
        assert call(ld, od, csr, rows, row_elems) == 0
    g.replay()
    torch.cuda.synchronize()
    assert same_bits(od, want)


def test_gate_readouts_refusals_leave_out_untouched(dev):
    rows, row_elems = 14, 21
    row_ptr, index, weight = make_csr(rows, 3)
    lines = make_lines(row_elems, 4)
    csr = csr_dev(row_ptr, index, weight, dev)
    lbuf, ld = placed(lines, 0, dev)
    obuf, od = placed(np.empty((rows, row_elems, 2), np.float32), 0, dev, fill=float("nan"))
    lib = L()
    lp, op, rp, ip, wp = ld.data_ptr(), od.data_ptr(), csr[0].data_ptr(), csr[1].data_ptr(), csr[2].data_ptr()

    def refused(want, args, word):
        assert lib.cine_scale(None, 1, 1.0, None) == EINVAL                   # another entry point's message, to be replaced
        assert lib.cine_gate_readouts(*args, stream()) == want, args
        msg = lib.cine_last_error()
        assert msg.startswith(b"cine_gate_readouts") and word in msg, msg
        torch.cuda.synchronize()
        assert bool(torch.isnan(od).all()) and guards_intact(obuf, od), "a refused call wrote"

    good = [lp, op, rp, ip, wp, N_LINES, rows, row_elems]
    for k in range(5):
        refused(EINVAL, good[:k] + [None] + good[k + 1:], b"null")
    refused(EINVAL, good[:6] + [0, row_elems], b"Invalid shapes")
    refused(EINVAL, good[:6] + [-3, row_elems], b"Invalid shapes")
    refused(EINVAL, good[:6] + [rows, 0], b"Invalid shapes")
    refused(EINVAL, good[:5] + [-1, rows, row_elems], b"Invalid shapes")
    refused(EINVAL, [lp + 4] + good[1:], b"8-byte aligned")
    refused(EINVAL, [lp, op + 4] + good[2:], b"8-byte aligned")
    refused(EINVAL, good[:2] + [rp + 2] + good[3:], b"4-byte aligned")
    # out inside lines, out ending inside lines, lines inside out
    refused(EINVAL, [lp, lp + 8 * row_elems] + good[2:], b"overlaps")
    refused(EINVAL, [lp, lp - 8] + good[2:], b"overlaps")
    refused(EINVAL, [op + 8, op] + good[2:5] + [1, rows, row_elems], b"overlaps")
    # the grid: one workgroup per row and chunk of 512 accesses, at most 2^31 - 1 (no readouts, so that nothing overlaps; refused
    # before the launch, the sizes stand for no memory)
    refused(EUNSUPPORTED, [op - 64, op] + good[2:5] + [0, 2 ** 31, 1], b"grid limit")
    refused(EUNSUPPORTED, [op - 64, op] + good[2:5] + [0, 2 ** 22, 512 * 512 + 1], b"grid limit")
    assert call(ld, od, csr, rows, row_elems) == 0                            # and the call works after every refusal
    torch.cuda.synchronize()
    check_gated(od.cpu().numpy(), lines, row_ptr, index, weight, "after the refusals")
