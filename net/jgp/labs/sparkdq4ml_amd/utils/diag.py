"""The one gate of the diagnostic kernel builds.

Some code generators can emit timing-only ABLATIONS of their kernels -- phases removed, results
wrong -- to attribute a kernel's time on the GPU box (``DQ4ML_CUT_ABLATE`` for the CSV field
cutter, ``ops/scancut.py``; ``DQ4ML_SCAN_ABL`` for the per-line scan, ``ops/scanfuse.py``), and
the cutter can carry per-phase clocks (``DQ4ML_CUT_STAMPS``: right results, but another kernel
than the product's).  They are profiling tools, never product behaviour: such a knob is honoured
only with ``DQ4ML_DIAG=1`` set as well, and set WITHOUT it the engine refuses to run rather than
return wrong numbers or time a kernel that is not the one it ships."""
from __future__ import annotations

import os

__all__ = ["ablation", "enabled", "flag"]


def enabled() -> bool:
    return os.environ.get("DQ4ML_DIAG", "0") == "1"


def ablation(name: str) -> int:
    """The bit mask of the wrong-result ablation env knob ``name`` (0: the real kernel)."""
    v = int(os.environ.get(name, "0") or 0)
    if v and not enabled():
        raise RuntimeError(f"{name}={v} builds a timing-only kernel with WRONG results; it is honoured only "
                           "for profiling, with DQ4ML_DIAG=1 set as well")
    return v


def flag(name: str) -> bool:
    """Whether the instrumented-build env knob ``name`` is on (``1``)."""
    on = os.environ.get(name, "0") == "1"
    if on and not enabled():
        raise RuntimeError(f"{name}=1 builds an instrumented kernel, not the product's; it is honoured only "
                           "for profiling, with DQ4ML_DIAG=1 set as well")
    return on
