"""Shared harness of the shape-by-shape kernel sweeps (test_grad_kernels.py, test_conv_fwd_kernels.py, test_transform_kernels.py): seeded case lists, guarded
device outputs, exact-size workspaces, the error bar and the worst error / bar report.  A plain module, not a conftest: the test files
import what they use."""
import numpy as np
import torch

BAR = 1e-5
BAR_CAP = 1e-4
LONG_REDUCTION = 100_000
GUARD = 8                                      # guard floats on each side of an output
GUARD_VALUE = 1234.5
WS_TAIL = 4096                                 # sentinel bytes behind a workspace


def sweep(seed, axes, count):
    """`count` seeded cases over `axes` (name -> list of values) in which every value of every axis appears: each axis walks a
    shuffled cycle of its values, so the combinations differ from case to case."""
    rs = np.random.RandomState(seed)
    cols = {}
    for name, vals in axes.items():
        order = []
        while len(order) < count:
            order.extend(rs.permutation(len(vals)).tolist())
        cols[name] = [vals[i] for i in order[:count]]
    return [{k: cols[k][i] for k in axes} for i in range(count)]


def cap_samples(n, per_sample, budget):
    """n reduced so that n * per_sample stays within budget (at least one sample): keeps the float64 references fast."""
    return max(1, min(n, budget // per_sample))


def case_id(c):
    return "-".join(f"{k}{int(v) if isinstance(v, bool) else v}" for k, v in c.items())


def hash_case(c):
    """A seed from the case's values (stable across runs, unlike hash())."""
    s = 0
    for v in c.values():
        s = (s * 1_000_003 + (int(v) if not isinstance(v, str) else sum(map(ord, v)))) % 2_147_483_000
    return s


def _bar(err_torch32, k):
    """The bar for a reduction of k terms: BAR, or above LONG_REDUCTION summed terms twice the error of torch's own float32
    result against the same reference, BAR at least and BAR_CAP at most."""
    return BAR if k <= LONG_REDUCTION else min(BAR_CAP, max(BAR, 2 * err_torch32))


class Worst:
    """The worst error / bar seen per entry point over a test module; record() asserts the bar."""

    def __init__(self):
        self.by_name = {}

    def __bool__(self):
        return bool(self.by_name)

    def record(self, what, err, bar, case):
        r = err / bar
        if r > self.by_name.get(what, (-1.0, None))[0]:
            self.by_name[what] = (r, case)
        assert err <= bar, f"{what} {case}: error {err:.3e} > bar {bar:.1e}"

    def report(self):
        print("\nworst error / bar per entry point:")
        for k in sorted(self.by_name):
            print(f"  {k:28s} {self.by_name[k][0]:.3f}  {self.by_name[k][1]}")


class Guarded:
    """A device tensor of `shape` at storage offset GUARD + off floats of a buffer whose other floats hold GUARD_VALUE."""

    def __init__(self, shape, off, dev, fill=None):
        self.n = int(np.prod(shape))
        self.lo = GUARD + off
        self.buf = torch.full((self.lo + self.n + GUARD,), GUARD_VALUE, device=dev)
        self.t = self.buf[self.lo:self.lo + self.n].view(shape)
        if fill is not None:
            self.t.copy_(fill)

    def ptr(self):
        return self.t.data_ptr()

    def intact(self):
        return bool((self.buf[:self.lo] == GUARD_VALUE).all()) and bool((self.buf[self.lo + self.n:] == GUARD_VALUE).all())


GUARD_INT = 0x5A5A5A5A


class GuardedInt:
    """Guarded for an int32 output (cine_acs_window's window): `n` ints between GUARD ints of GUARD_INT on each side."""

    def __init__(self, n, dev, fill=-1):
        self.n = n
        self.buf = torch.full((2 * GUARD + n,), GUARD_INT, dtype=torch.int32, device=dev)
        self.t = self.buf[GUARD:GUARD + n]
        self.t.fill_(fill)

    def ptr(self):
        return self.t.data_ptr()

    def intact(self):
        return bool((self.buf[:GUARD] == GUARD_INT).all()) and bool((self.buf[GUARD + self.n:] == GUARD_INT).all())


def same_bits(a, b):
    """Bit equality of two float32 tensors (NaN-safe, and -0 differs from +0)."""
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def view_at(x, off, dev):
    """x on the device at storage offset off (a pointer 4 * off bytes past an aligned allocation)."""
    return Guarded(x.shape, off, dev, x.to(dev)).t


class Workspace:
    """Exactly `nbytes` of workspace, carved from a larger buffer whose tail holds a sentinel pattern."""

    def __init__(self, nbytes, dev):
        self.nbytes = int(nbytes)
        self.tail = (torch.arange(WS_TAIL, dtype=torch.int64) * 37 % 251).to(torch.uint8).to(dev)
        self.buf = torch.zeros(self.nbytes + WS_TAIL, dtype=torch.uint8, device=dev)
        self.buf[self.nbytes:] = self.tail

    def ptr(self):
        return self.buf.data_ptr()

    def intact(self):
        return torch.equal(self.buf[self.nbytes:], self.tail)
