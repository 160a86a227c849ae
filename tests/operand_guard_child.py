"""Child runner of tests/test_operand_containment.py: ``python -m tests.operand_guard_child <family> [--after <case>]``.

Loads the lane-emulator build (never the product library), runs every case of the family on guarded operands (tests/guarded.py) and prints

    BEGIN <case> <side>
    END <case> <side> guarded=<operands placed> allocs=<allocations intercepted> gap=<largest gap, bytes> seconds=<wall time> calls=<a,b,...>

(``calls``: the ``pcdm_*`` entry points the case reached, recorded by a proxy in front of the library), flushed, so that the parent knows
which case a SIGSEGV belongs to (``faulthandler`` prints the Python stack to stderr).  ``--after``: skip every case up to and including that
one (the parent restarts the child behind a finding)."""
from __future__ import annotations

import argparse
import faulthandler
import sys
import time


class Recorder:
    """in front of the bound library: notes the name of every entry point looked up (every call goes through ``_lib.lib().<name>``)"""

    def __init__(self, lib):
        self._lib, self.names = lib, set()

    def __getattr__(self, name):
        self.names.add(name)
        return getattr(self._lib, name)


def main(argv=None) -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("family")
    ap.add_argument("--after", default=None)
    a = ap.parse_args(argv)
    faulthandler.enable()
    from pcdms_amd import _lib
    from tests.emu import build_emu
    _lib.use_library(build_emu.load())
    assert _lib.is_emulator()
    rec = _lib._lib = Recorder(_lib._lib)
    from tests import test_operand_containment as T
    names = [n for n, c in T.CASES.items() if c.family == a.family]
    if not names:
        print(f"no such family: {a.family}", file=sys.stderr)
        return 2
    if a.after is not None:
        names = names[names.index(a.after) + 1:]
    for name in names:
        for side in T.CASES[name].sides:
            print(f"BEGIN {name} {side}", flush=True)
            t0 = time.perf_counter()
            rec.names.clear()
            count, allocs, gap = T.run_guarded(name, side)
            calls = ",".join(sorted(n for n in rec.names if n.startswith("pcdm_"))) or "-"
            print(f"END {name} {side} guarded={count} allocs={allocs} gap={gap} seconds={time.perf_counter() - t0:.3f} calls={calls}", flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
