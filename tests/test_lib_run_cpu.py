"""_lib.run and _lib.cptr, the two helpers every host-side launch goes through, against a fake library object (no GPU, no
loaded library): the stream goes last, the entry point is looked up when called, and the return code is read as the C ABI
defines it (0 done, 1 "not for this shape, nothing done", negative an error with cm_last_error's text)."""
import pytest
import torch


class _FakeLib:
    def __init__(self):
        self.got, self.rc = [], 0

    def cm_thing(self, *a):
        self.got.append(a)
        return self.rc

    def cm_last_error(self):
        return b"the library's own words"


def test_run_and_cptr(monkeypatch):
    from com_marl_amd import _lib as L
    fake = _FakeLib()
    monkeypatch.setattr(L, "lib", lambda: fake)
    monkeypatch.setattr(L, "current_stream", lambda: 0x5EED)

    assert L.run("cm_thing", 1, None, "x") is True
    assert fake.got == [(1, None, "x", 0x5EED)]                              # the stream is the last argument
    assert L.run("cm_thing", maybe=True) is True and fake.got[-1] == (0x5EED,)

    later = _FakeLib()                                                       # installed after import: seen, looked up per call
    monkeypatch.setattr(L, "lib", lambda: later)
    assert L.run("cm_thing", 2) is True and later.got == [(2, 0x5EED)] and len(fake.got) == 2
    seen = []
    later.cm_thing = lambda *a: seen.append(a) or 0                          # and a replaced entry point of the same object
    assert L.run("cm_thing", 3) is True and seen == [(3, 0x5EED)]
    del later.cm_thing

    later.rc = 1
    assert L.run("cm_thing", 4, maybe=True) is False                         # "not for this shape": no error
    with pytest.raises(L.CommarlError, match=r"cm_thing failed \(1\): the library's own words"):
        L.run("cm_thing", 4)
    later.rc = -3
    for maybe in (False, True):
        with pytest.raises(L.CommarlError, match=r"cm_thing failed \(-3\)"):
            L.run("cm_thing", 5, maybe=maybe)
    with pytest.raises(AttributeError):
        L.run("cm_no_such_entry_point")

    assert L.cptr(None) is None
    t = torch.arange(12, dtype=torch.float32).reshape(3, 4)
    assert L.cptr(t) == t.data_ptr() == L.ptr(t)
    v = t.t()                                                                # not contiguous: a contiguous copy's address
    assert not v.is_contiguous() and L.cptr(v) not in (None, t.data_ptr())
    with pytest.raises(AssertionError):
        L.ptr(v)
