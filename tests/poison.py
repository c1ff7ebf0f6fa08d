"""Fresh-memory poisoning for the tests (a helper module, not a conftest).

The library takes every scratch, saved-state and output buffer uninitialised: `torch.empty`, `torch.empty_like`,
`Tensor.new_empty` and `_C.scratch` (itself a `torch.empty`).  A fresh process gets zero pages and the caching allocator
hands a test its own previous buffers back, so a word the library reads or returns without writing it first usually holds
a benign value under test and another kernel's data in training.  `poisoned(pattern)` makes the difference visible: while
it is active, every tensor those three calls return is filled with `pattern` first.

    with poisoned("nan") as p:
        out = op(...)
    assert p.bytes > 0

Patterns, applied to the BYTES of the buffer (the whole storage behind the tensor, so dtype and shape do not matter):
  zeros   every byte 0: the baseline all other runs are compared with
  one     the storage seen as little-endian int64 words, each 1, trailing bytes 0: an int32 / int64 slot read as an index or
          a count sees 0 or 1 (in bounds wherever anything is), a float slot a denormal or 0
  nan     every byte 0xFF: float / double NaN, int -1, uint32 2^32 - 1
bool tensors get False under `zeros` and the byte 0x01 under both other patterns: a bool that holds 0xFF is outside torch's
own contract for nonzero() and indexing.

`check(fn)` is the ladder every test uses: fn() unpatched, then under zeros, one, nan IN THAT ORDER, each result compared
bit for bit with the zeros run, and the ladder STOPS at the first pattern that differs.  The order is deliberate: the
library's integer scratch holds indices, an uninitialised index read shows under `one` as a wrong result (0 or 1 is a
valid index) and fails the test there, so the -1 of `nan` is never handed to that kernel.  That is the most cautious order
available, not a guarantee.

What the patch covers: the attributes `torch.empty`, `torch.empty_like` and `torch.Tensor.new_empty`, i.e. every call made
through the module / class attribute at call time.  All allocation sites of splatco_amd/*.py are of that kind (no
`from torch import empty`, no `empty_strided`, no `resize_`).  Not covered, by construction:
  * zero-size tensors (skipped: nothing to fill), e.g. the `torch.empty(0).set_(storage, ...)` view of multiview.py and the
    empty leaf of renderer.py;
  * tensors torch allocates inside its own C++ operators (cat, nonzero, arithmetic results): those are written by the
    operator that makes them;
  * `torch.empty(..., out=t)`: t is the caller's.
"""
import contextlib

import torch

PATTERNS = ("zeros", "one", "nan")


class Poison:
    """What a `poisoned` block filled: `count` allocations, `bytes` bytes."""

    def __init__(self, pattern):
        self.pattern, self.count, self.bytes = pattern, 0, 0


def _fill(t, pattern, orig_empty):
    """Fill the storage behind `t` with `pattern`.  Returns the number of bytes written."""
    st = t.untyped_storage()
    n = st.nbytes()
    with torch.no_grad():
        raw = orig_empty(0, dtype=torch.uint8, device=t.device).set_(st, 0, (n,))
        if t.dtype == torch.bool:
            raw.fill_(0 if pattern == "zeros" else 1)
        elif pattern == "zeros":
            raw.zero_()
        elif pattern == "nan":
            raw.fill_(0xFF)
        else:
            words = n // 8
            if words:
                raw[:words * 8].view(torch.int64).fill_(1)
            if n > words * 8:
                raw[words * 8:].zero_()
    return n


@contextlib.contextmanager
def poisoned(pattern):
    if pattern not in PATTERNS:
        raise ValueError(f"poisoned: pattern {pattern!r} is not one of {PATTERNS}")
    state = Poison(pattern)
    saved = (torch.empty, torch.empty_like, torch.Tensor.new_empty)
    orig_empty = saved[0]

    def wrap(orig):
        def made(*args, **kwargs):
            t = orig(*args, **kwargs)
            if isinstance(t, torch.Tensor) and t.numel() > 0 and kwargs.get("out") is None:
                state.bytes += _fill(t, pattern, orig_empty)
                state.count += 1
            return t
        made.__name__ = getattr(orig, "__name__", "empty")
        return made

    torch.empty, torch.empty_like, torch.Tensor.new_empty = (wrap(f) for f in saved)
    try:
        yield state
    finally:
        torch.empty, torch.empty_like, torch.Tensor.new_empty = saved


def _bits(t):
    """The tensor's logical elements as integers, so that NaN payloads and -0.0 count."""
    t = t.detach().contiguous()
    if t.dtype == torch.bool:
        return t.to(torch.uint8).flatten()
    if t.numel() == 0:
        return t.flatten()
    view = torch.int32 if t.element_size() % 4 == 0 else torch.uint8
    return t.reshape(-1).view(view)


def same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and bool(torch.equal(_bits(a), _bits(b)))


def check(fn, finite=True, sync=None, unpatched=True):
    """Run fn() unpatched, then under zeros, one and nan; fn returns a flat list of tensors (outputs and gradients, logical
    views only).  Every run must give the bits of the zeros run; the first pattern that differs raises AssertionError and
    the later patterns are not run.  With finite=True every floating-point output must also be finite in every run.
    unpatched=False leaves the first run out (the helper's own tests: what an unpatched leaky operator reads is arbitrary).
    Returns {pattern: Poison} (and the zeros run's outputs under "outputs"), each with bytes > 0 asserted."""
    def run(pattern):
        if pattern is None:
            out = list(fn())
            state = None
        else:
            with poisoned(pattern) as state:
                out = list(fn())
        if sync is not None:
            sync()
        return [o.detach().clone() for o in out], state

    def all_finite(out, pattern):
        if finite:
            for i, o in enumerate(out):
                if o.is_floating_point():
                    assert bool(torch.isfinite(o).all()), f"output {i} is not finite under {pattern}"

    plain = run(None)[0] if unpatched else None
    base, filled = run("zeros")
    assert filled.bytes > 0 and filled.count > 0, "the case allocates nothing through torch.empty: it checks nothing"
    report = {"outputs": base, "zeros": filled}
    assert plain is None or len(plain) == len(base)
    for i, (a, b) in enumerate(zip(plain or (), base)):
        assert same_bits(a, b), f"output {i} differs between the unpatched run and zero-filled buffers"
    all_finite(base, "zeros")
    for pattern in ("one", "nan"):
        got, filled = run(pattern)
        assert filled.bytes > 0
        assert len(got) == len(base)
        for i, (a, b) in enumerate(zip(got, base)):
            if not same_bits(a, b):
                n = int((_bits(a) != _bits(b)).sum()) if a.shape == b.shape and a.dtype == b.dtype else -1
                raise AssertionError(f"output {i} ({tuple(b.shape)} {b.dtype}) depends on what its buffers held: "
                                     f"{n} words differ under '{pattern}' (ladder stopped here)")
        all_finite(got, pattern)
        report[pattern] = filled
    return report
