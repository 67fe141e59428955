"""TEST INFRASTRUCTURE ONLY -- the twin harness of tests/test_gpu_streams.py.

A scenario is a function ``scenario(T, ...)`` of a ``Twin``.  It is run twice:

* twin A on the null stream, as every other GPU test runs: ``Twin(None, None)``;
* twin B inside ``torch.cuda.stream(s)`` for a side stream ``s``: ``Twin(delay, s)``.

Inside a scenario every input a library call consumes is first staged on the device
(``T.dev``), the device is drained once (``T.ready``), and from then on an input reaches its
buffer only through ``T.put(dst, src)``: in twin B a ``Delay`` and then the device-to-device
``dst.copy_(src)``, both on ``s``, with no host synchronisation before the library call that
follows.  (A copy from pageable host memory would block the host until the delay has run and so
hide what the twins are there to show.)  ``dst`` held other valid contents before, so a piece of
the call that is not ordered after ``s`` reads those and the twins differ.  ``same`` compares two
results bit for bit: no tolerance anywhere.
"""
import contextlib

import numpy as np
import torch


class Delay:
    """Plain torch work on the current stream: ``reps`` square f32 matmuls into a scratch tensor.
    The operands are small enough that every product stays finite."""

    def __init__(self, n=4096, reps=4):
        self.reps = reps
        self.a = torch.full((n, n), 1.0 / n, dtype=torch.float32, device="cuda")
        self.b = torch.full((n, n), 0.5, dtype=torch.float32, device="cuda")
        self.c = torch.zeros((n, n), dtype=torch.float32, device="cuda")
        torch.cuda.synchronize()

    def __call__(self):
        for _ in range(self.reps):
            torch.mm(self.a, self.b, out=self.c)

    def busy_seconds(self, stream):
        """The event-timed duration of one delay on ``stream`` (after a warm-up delay)."""
        with torch.cuda.stream(stream):
            self()
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0.record()
            self()
            t1.record()
        t1.synchronize()
        return t0.elapsed_time(t1) * 1e-3


class Twin:
    """One run of a scenario: on the null stream (``stream`` None) or on a side stream."""

    def __init__(self, delay=None, stream=None):
        self.delay_fn = delay
        self.stream = stream

    @property
    def side(self):
        return self.stream is not None

    def on(self):
        """The context the twin's torch work and library calls run in."""
        return torch.cuda.stream(self.stream) if self.side else contextlib.nullcontext()

    def dev(self, a):
        """A host array on the device (setup: a pageable copy blocks the host)."""
        return torch.as_tensor(np.ascontiguousarray(a), device="cuda")

    def ready(self):
        """End of the setup: every staged tensor is written, whatever stream wrote it."""
        torch.cuda.synchronize()

    def delay(self):
        if self.side:
            self.delay_fn()

    def put(self, dst, src):
        """The producer: a delay (twin B), then the real input over ``dst``'s other contents."""
        assert src.is_cuda and dst.is_cuda and src.dtype == dst.dtype and src.numel() == dst.numel()
        self.delay()
        dst.copy_(src.view(dst.shape))


def run(scenario, T, *args, **kw):
    with T.on():
        out = scenario(T, *args, **kw)
    torch.cuda.synchronize()
    return out


def twins(scenario, delay, *args, stream=None, **kw):
    """(twin A's result, twin B's) of a scenario; B on ``stream`` or on a fresh side stream."""
    a = run(scenario, Twin(), *args, **kw)
    b = run(scenario, Twin(delay, stream if stream is not None else torch.cuda.Stream()), *args, **kw)
    return a, b


def _leaves(x, path):
    if isinstance(x, dict):
        for k in sorted(x, key=str):
            yield from _leaves(x[k], f"{path}.{k}")
    elif isinstance(x, (list, tuple)):
        for k, v in enumerate(x):
            yield from _leaves(v, f"{path}[{k}]")
    elif isinstance(x, (bytes, bytearray)):
        yield path, np.frombuffer(bytes(x), np.uint8)
    elif x is None or isinstance(x, (str, bool)):
        yield path, np.frombuffer(repr(x).encode(), np.uint8)
    else:
        if isinstance(x, torch.Tensor):
            x = x.cpu().numpy()
        a = np.ascontiguousarray(x)
        assert a.dtype != object, (path, type(x))
        yield f"{path}{a.dtype}{list(a.shape)}", a.reshape(-1).view(np.uint8)


def same(a, b):
    """Bit for bit: the same tree of dicts, lists and arrays, every leaf's bytes equal (so a NaN
    equals itself and -0.0 differs from 0.0)."""
    la, lb = list(_leaves(a, "")), list(_leaves(b, ""))
    assert [p for p, _ in la] == [p for p, _ in lb], "the twins' results differ in shape"
    for (p, x), (_, y) in zip(la, lb):
        if not np.array_equal(x, y):
            d = np.flatnonzero(x != y)
            raise AssertionError(f"twin B differs from twin A at {p}: {len(d)} of {x.size} bytes, the first at {d[0]}")


def differs(a, b):
    try:
        same(a, b)
    except AssertionError:
        return True
    return False
