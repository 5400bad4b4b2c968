"""The engine keeps Python's cyclic collector out of a graph capture (sy11.engine._no_gc_while_capturing): garbage that exists
before the capture is finalised on entry, nothing is finalised inside, and the collector's previous state comes back."""
import gc

import pytest

from sy11.engine import _no_gc_while_capturing


class _Cycle:
    def __init__(self, log, name):
        self.me, self.log, self.name = self, log, name

    def __del__(self):
        self.log.append(self.name)


def test_garbage_is_collected_on_entry_and_not_inside():
    log = []
    assert gc.isenabled()
    _Cycle(log, "before")
    with _no_gc_while_capturing():
        assert log == ["before"] and not gc.isenabled()
        for i in range(3 * gc.get_threshold()[0]):          # enough allocations to trigger several automatic collections
            _Cycle(log, "inside")
        assert log == ["before"]
    assert gc.isenabled()
    gc.collect()
    assert log.count("inside") == 3 * gc.get_threshold()[0]


def test_collector_state_is_restored():
    gc.disable()
    try:
        with _no_gc_while_capturing():
            assert not gc.isenabled()
        assert not gc.isenabled()
    finally:
        gc.enable()
    with pytest.raises(RuntimeError):
        with _no_gc_while_capturing():
            raise RuntimeError("capture failed")
    assert gc.isenabled()
