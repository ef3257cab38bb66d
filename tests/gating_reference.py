"""The float64 restatement of cine_gate_readouts that tests/test_gating_kernel.py and tests/test_gating_pipeline.py share, and the bar
it is held to.  Plain loops over the CSR arrays; nothing here knows about chunks, lanes or access widths."""
import numpy as np


def gate_ref64(lines, row_ptr, index, weight):
    """lines (n_lines, row_elems, 2) float32, the CSR arrays as numpy -> (ref, mag, count): ref (rows, row_elems, 2) float64 with
    ref[r] = sum_j weight[j] lines[index[j]] (every product of two float32 values is exact in float64), mag the same sum over
    |weight[j] lines[index[j]]| per real component, count (rows,) the entries of each row."""
    rows = row_ptr.shape[0] - 1
    x = lines.astype(np.float64)
    ref = np.zeros((rows,) + lines.shape[1:], dtype=np.float64)
    mag = np.zeros_like(ref)
    for r in range(rows):
        for j in range(int(row_ptr[r]), int(row_ptr[r + 1])):
            term = float(weight[j]) * x[int(index[j])]
            ref[r] += term
            mag[r] += np.abs(term)
    return ref, mag, np.diff(row_ptr.astype(np.int64))


def check_gated(out, lines, row_ptr, index, weight, what=""):
    """The three bars of the kernel's contract on out (rows, row_elems, 2) float32 (numpy):
      * a row without entries is exactly 0;
      * a row with the single weight 1.0 holds its line's bits (the data are finite);
      * otherwise, per real component, |out - ref64| <= (k + 1) 2^-24 sum_j |w_j x_j| for a row of k entries: one rounding per
        term -- the product, then k - 1 fused multiply-adds, each rounding a partial sum no larger than the sum of magnitudes.
    Returns the worst error as a fraction of its bar."""
    ref, mag, count = gate_ref64(lines, row_ptr, index, weight)
    assert np.isfinite(out).all(), f"{what}: a value is not finite"
    worst = 0.0
    for r in range(count.shape[0]):
        k = int(count[r])
        j0 = int(row_ptr[r])
        if k == 0:
            assert not out[r].view(np.int32).any(), f"{what}: empty row {r} is not +0"
        elif k == 1 and weight[j0] == np.float32(1.0):
            assert np.array_equal(out[r].view(np.int32), lines[int(index[j0])].view(np.int32)), f"{what}: row {r} is not its line, bit for bit"
        else:
            bar = (k + 1) * 2.0 ** -24 * mag[r]
            err = np.abs(out[r].astype(np.float64) - ref[r])
            assert (err <= bar).all(), f"{what}: row {r} ({k} entries): error {float((err - bar).max()):.3e} above its bar"
            worst = max(worst, float((err / np.maximum(bar, 1e-300)).max()))
    return worst
