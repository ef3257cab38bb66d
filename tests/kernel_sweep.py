"""Shared harness of the shape-by-shape kernel sweeps (test_grad_kernels.py, test_conv_fwd_kernels.py, test_transform_kernels.py, test_cg_kernels.py):
seeded case lists, guarded device outputs, exact-size workspaces, the error bar, the worst error / bar report and the operands of one call
through the C ABI (Call, twice, at_offsets, refused).  A plain module, not a conftest: the test files
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


class GuardedF64:
    """Guarded for a float64 output (cine_image_metrics' out, the complex128 Gram matrices as double pairs): `n` doubles, NaN, between
    GUARD doubles of GUARD_VALUE at least on each side, at a storage offset of `off` doubles (an even `off` keeps 16-byte alignment)."""

    def __init__(self, n, dev, off=0):
        self.n = n
        self.lo = GUARD + off
        self.buf = torch.full((self.lo + n + GUARD,), GUARD_VALUE, dtype=torch.float64, device=dev)
        self.t = self.buf[self.lo:self.lo + n]
        self.t.fill_(float("nan"))

    def ptr(self):
        return self.t.data_ptr()

    def intact(self):
        return bool((self.buf[:self.lo] == GUARD_VALUE).all()) and bool((self.buf[self.lo + self.n:] == GUARD_VALUE).all())


def same_bits(a, b):
    """Bit equality of two float32 tensors (NaN-safe, and -0 differs from +0)."""
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def view_at(x, off, dev):
    """x on the device at storage offset off (a pointer 4 * off bytes past an aligned allocation)."""
    return Guarded(x.shape, off, dev, x.to(dev)).t


class Workspace:
    """Exactly `nbytes` of workspace, carved from a larger buffer whose tail holds a sentinel pattern.  past256: the base pointer lies that
    many bytes past a 256-byte boundary (None: the allocation's own base), behind a head of the same pattern."""

    def __init__(self, nbytes, dev, past256=None):
        self.nbytes = int(nbytes)
        self.tail = (torch.arange(WS_TAIL, dtype=torch.int64) * 37 % 251).to(torch.uint8).to(dev)
        if past256 is None:
            self.lo = 0
            self.buf = torch.zeros(self.nbytes + WS_TAIL, dtype=torch.uint8, device=dev)
        else:
            self.whole = torch.zeros(512 + self.nbytes + WS_TAIL, dtype=torch.uint8, device=dev)
            self.lo = (-self.whole.data_ptr()) % 256 + 256 + past256
            self.whole[:self.lo] = self.tail[:self.lo]
            self.buf = self.whole[self.lo:self.lo + self.nbytes + WS_TAIL]
            assert self.buf.data_ptr() % 256 == past256
        self.buf[self.nbytes:] = self.tail

    def ptr(self):
        return self.buf.data_ptr()

    def intact(self):
        return torch.equal(self.buf[self.nbytes:], self.tail) and (self.lo == 0 or torch.equal(self.whole[:self.lo], self.tail[:self.lo]))


# ================================================================== one call through the C ABI (the GPU tests of the sweeps)
NAN = float("nan")
EINVAL, EUNSUPPORTED, EWORKSPACE = -1, -2, -3


def L():
    from cine_hip._lib import lib
    return lib()


def check(code, what):
    from cine_hip._lib import check as _check
    _check(code, what)


def stream():
    return torch.cuda.current_stream().cuda_stream


def ptr(t):
    return None if t is None else t.data_ptr()


def unchanged(t, keep):
    return same_bits(t, keep) if t.dtype == torch.float32 else torch.equal(t, keep)


class Call:
    """The operands of one call with every float pointer at storage offset `off` floats: inputs are kept to prove them unchanged, outputs
    sit between guard floats and are prefilled with NaN, a workspace has exactly the size asked for."""

    def __init__(self, dev, off):
        self.dev, self.off, self.ins, self.outs, self.wss = dev, off, [], [], []

    def inp(self, x):
        if x is None:
            return None
        t = view_at(x.contiguous(), self.off, self.dev)
        self.ins.append((t, t.clone()))
        return t

    def inp_among_nan(self, x):
        """inp with NaN in place of the guard value on both sides: a read outside the operand spoils the result."""
        x = x.contiguous()
        buf = torch.full((GUARD + self.off + x.numel() + GUARD,), NAN, device=self.dev)
        t = buf[GUARD + self.off:GUARD + self.off + x.numel()].view(x.shape)
        t.copy_(x)
        self.ins.append((buf, buf.clone()))
        return t

    def raw(self, x):
        """uint8 masks, int32 windows, the one float of lambda_dev: at their allocation's base."""
        t = x.contiguous().to(self.dev)
        self.ins.append((t, t.clone()))
        return t

    def lam(self, v):
        return None if v is None else self.raw(torch.tensor([v], dtype=torch.float32))

    def out(self, shape, fill=None):
        """A pure output (NaN prefill) or, with `fill`, an operand updated in place."""
        g = Guarded(tuple(shape), self.off, self.dev)
        if fill is None:
            g.t.fill_(NAN)
        else:
            g.t.copy_(fill)
        self.outs.append(g)
        return g

    def out64(self, n):
        """A pure float64 output of n doubles (NaN prefill) at the call's storage offset: `off` floats are off / 2 doubles."""
        assert self.off % 2 == 0
        g = GuardedF64(n, self.dev, self.off // 2)
        self.outs.append(g)
        return g

    def ws(self, nbytes, past256=None, fill=0xFF):
        if not nbytes:
            return None
        w = Workspace(nbytes, self.dev, past256)
        w.buf[:w.nbytes] = fill                     # 0xFF: NaN bit patterns; the result must not depend on what the workspace held
        self.wss.append(w)
        return w

    def finish(self, what):
        torch.cuda.synchronize()
        for g in self.outs:
            assert g.intact(), f"{what}: write outside an output"
        for w in self.wss:
            assert w.intact(), f"{what}: write past the workspace"
        for t, keep in self.ins:
            assert unchanged(t, keep), f"{what}: an input changed"


def twice(dev, off, body, what):
    """body(Call) makes the call on fresh operands and returns its output tensors: twice, the same bits; returns them on the CPU."""
    res = []
    for _ in range(2):
        k = Call(dev, off)
        outs = body(k)
        k.finish(what)
        res.append([o.clone() for o in outs])
    for a, b in zip(*res):
        assert same_bits(a, b), f"{what}: a second call gives other bits"
    return [o.cpu() for o in res[0]]


def at_offsets(dev, offs, body, what):
    """twice at every storage offset of offs; all give the bits of the first."""
    res = [twice(dev, off, body, what) for off in offs]
    for r in res[1:]:
        for a, b in zip(res[0], r):
            assert same_bits(a, b), f"{what}: other bits at a storage offset of {offs[1]} floats"
    return res[0]


def refused(call, want, k, what, name=None):
    """call() returns `want`, leaves a message of its own -- it names the entry point (`name`, by default the first word of `what`) and
    replaces the message of another entry point's refusal made just before -- and writes nothing: guards intact, every output and
    in-place operand holds the bits it held (a pure output is still NaN), inputs unchanged."""
    name = name or what.split()[0]
    assert name.startswith("cine_") and name != "cine_scale", what
    assert L().cine_scale(None, 1, 1.0, None) == EINVAL and L().cine_last_error().startswith(b"cine_scale")
    before = [g.buf.clone() for g in k.outs]
    code = call()
    assert code == want, f"{what}: returned {code}, expected {want}"
    msg = L().cine_last_error().decode(errors="replace")
    assert msg.startswith(name), f"{what}: the message is not this call's: {msg!r}"
    k.finish(what)
    for g, keep in zip(k.outs, before):
        assert same_bits(g.buf, keep), f"{what}: an output was written before the refusal"
