"""A recording stand-in for the loaded library (com_marl_amd._lib.lib()) and the fixture that installs it: the tests that
assert WHICH C entry points a route launched import `spy` from here.  The package looks every entry point up on _lib.lib() at
call time (_lib.run, _lib.launch), so a stand-in installed after import sees every launch."""
import pytest


class _Call(str):
    """The name of one cm_* call, with the arguments it got as `.args`."""


class _Spy:
    """Stands in for the loaded library: records every cm_* call (`calls`: the names, in order, each a _Call), then makes it."""

    def __init__(self, real):
        self._real, self.calls = real, []

    def __getattr__(self, name):
        fn = getattr(self._real, name)
        if not name.startswith("cm_") or name == "cm_last_error":
            return fn

        def call(*a):
            rec = _Call(name)
            rec.args = a
            self.calls.append(rec)
            return fn(*a)
        return call

    def names(self):
        return set(self.calls)

    def count(self, name):
        return self.calls.count(name)

    def replicas(self):
        """The bias_replicas arguments the cm_masked_agg_backward_r calls got."""
        return {c.args[14] for c in self.calls if c == "cm_masked_agg_backward_r"}


@pytest.fixture
def spy(monkeypatch):
    from com_marl_amd import _lib as L
    s = _Spy(L.lib())
    monkeypatch.setattr(L, "lib", lambda: s)
    return s
