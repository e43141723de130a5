"""Operands derived from fp32 master parameters (packed 16-bit weights, LayerNorm folds, low-rank and lookup tables), cached on the
module that uses them until the operand type, the caller's spec or a source's (device, address, in-place version) changes."""
import contextlib
import contextvars

import torch

from . import ops

BUILDS = 0                      # cache misses so far (read by the tests)
_STREAMS = contextvars.ContextVar("vf_build_streams", default=None)


@contextlib.contextmanager
def build_streams(main, side):
    """The modulator's two-stream section: a miss inside builds on `main`, with the two streams joined around it."""
    token = _STREAMS.set((main, side))
    try:
        yield
    finally:
        _STREAMS.reset(token)


def _versions(sources):
    return tuple((t.device, t.data_ptr(), t._version) for t in sources if t is not None)


def derived(owner, slot: str, sources, build, *spec):
    """build()'s value, kept in owner.__dict__[slot] under the key (ops.cdt(), *spec, versions of the non-None sources);
    a new key replaces that slot's entry and nothing else."""
    key = (ops.cdt(),) + spec + _versions(sources)
    hit = owner.__dict__.get(slot)
    if hit is not None and hit[0] == key:
        return hit[1]
    global BUILDS
    BUILDS += 1
    streams = _STREAMS.get()
    with torch.no_grad():
        if streams is None:
            value = build()
        else:
            # Never beside the other stream's kernels: torch's are not built without packed-fp32 instructions (csrc/build.py).
            # Replacing is safe too: entries are allocated from and freed into main's pool, the old one after main has waited
            # for all side work so far, and main waits for side at the end of every forward, so a freed block is never reused
            # while a side-stream kernel may still read it.
            main, side = streams
            main.wait_stream(side)
            with torch.cuda.stream(main):
                value = build()
            side.wait_stream(main)
    owner.__dict__[slot] = (key, value)
    return value


def built_from(owner, slot: str, sources, *spec) -> bool:
    """The entry in `slot` was built from these versions of `sources` and this spec, in whichever operand type."""
    hit = owner.__dict__.get(slot)
    return hit is not None and hit[0][1:] == spec + _versions(sources)
