"""CPU tests of the two pieces every wrapper of engine.py stands on: `_native.call`, which names a library function once and raises
when it does not return MPE_OK, and `engine._Handle`, the one close() / __del__ of the classes that own a native object.  The typed
constants of the header (`((int)841)`) reach _native through the generated _abi.py.  No library call here touches a device."""
import ctypes
import os
import re
import sys
import types

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HANDLE_OWNERS = ["Context", "ModSet", "PaillierKeys", "Statements", "Gg20Keys", "Gg20Session", "WrapKey", "PresigPool", "Comm", "Gg20Pipeline",
                 "Gg18Wallet"]
TYPED = ["SEAL_MAGIC", "SEAL_REFUSED", "SEAL_MAX_WORDS", "SEAL_KIND_PRESIG", "SEAL_KIND_KEYSHARE", "SEAL_KIND_USER", "GG20_KEYSHARE_WORDS",
         "GG20_STATUS_BAD_TWEAK", "SHA512_MAX_MSG_BYTES", "BIP32_MAX_DEPTH", "BIP32_STATUS_HARDENED", "BIP32_STATUS_INVALID", "BIP32_STATUS_DEPTH"]


@pytest.fixture
def stand_in(monkeypatch):
    """_native.lib replaced by an object whose mpe_sync / mpe_ctx_set_option return what the test sets; a fresh call namespace over it"""
    from multi_party_ecdsa_amd import _native as N
    seen = []

    def fn(*args):
        seen.append(args)
        return lib.rc
    lib = types.SimpleNamespace(rc=0, seen=seen, mpe_sync=fn, mpe_ctx_set_option=fn, mpe_last_error=lambda: b"stand-in says no")
    monkeypatch.setattr(N, "lib", lib)
    return N, N._Call(), lib


def test_call_passes_a_status_of_ok_through_silently(stand_in):
    N, call, lib = stand_in
    assert call.mpe_sync(1, 2) is None and lib.seen == [(1, 2)]
    assert call.mpe_sync(3) is None and lib.seen == [(1, 2), (3,)]                 # the cached wrapper still calls


def test_call_raises_with_the_name_of_the_function_or_with_what(stand_in):
    N, call, lib = stand_in
    lib.rc = N.MPE_E_ARG
    with pytest.raises(N.MpeError) as e:
        call.mpe_sync(None, None)
    assert re.search(r"^mpe_sync failed: rc=-1 \(", str(e.value)) and str(e.value) == "mpe_sync failed: rc=-1 (stand-in says no)"
    with pytest.raises(N.MpeError) as e:
        call.mpe_ctx_set_option(None, b"k", b"v", what="mpe_ctx_set_option(k)")
    assert re.search(r"^mpe_ctx_set_option\(k\) failed: rc=-1 \(", str(e.value))
    assert lib.seen == [(None, None), (None, b"k", b"v")]                            # `what` is not passed on to the library
    lib.rc = N.MPE_E_NOMEM
    with pytest.raises(N.MpeError, match=r"^mpe_sync failed: rc=-3 \("):
        call.mpe_sync(None, None)


def test_call_is_check_over_the_real_library():
    """the same message as check() gives, from a library call that refuses its NULL arguments before any HIP call"""
    from multi_party_ecdsa_amd import _native as N
    with pytest.raises(N.MpeError) as e:
        N.call.mpe_ctx_create(None, 0)
    with pytest.raises(N.MpeError) as want:
        N.check(N.lib.mpe_ctx_create(None, 0), "mpe_ctx_create")
    assert str(e.value) == str(want.value) and re.search(r"^mpe_ctx_create failed: rc=-1 \(", str(e.value))


def test_call_refuses_a_function_that_returns_no_status():
    from multi_party_ecdsa_amd import _abi, _native as N
    assert _abi.SIGNATURES["mpe_last_error"][0] is ctypes.c_char_p and _abi.SIGNATURES["mpe_encoding_default"][0] is None
    for name in ("mpe_last_error", "mpe_version", "mpe_encoding_default"):
        with pytest.raises(TypeError, match=name):
            getattr(N.call, name)
        assert name not in vars(N.call)                                                # refused at every use, not only the first
    with pytest.raises(AttributeError):
        N.call.mpe_no_such_function
    assert isinstance(N.lib.mpe_last_error(), bytes)                                   # lib stays raw


def test_handle_close_destroys_once_and_del_never_raises():
    from multi_party_ecdsa_amd import engine as E

    class Owner(E._Handle):
        destroyed = []

        def __init__(self, fail):
            if fail:
                raise E.N_.MpeError("refused")
            self.h = ctypes.c_void_p(1234)

        def _destroy(self):
            self.destroyed.append(self.h.value)
    o = Owner(False)
    o.close()
    assert Owner.destroyed == [1234] and o.h is None
    o.close()
    o.__del__()                                                                        # after close(): nothing
    assert Owner.destroyed == [1234]
    # a constructor that raised before it set h: the object is closable, __del__ destroys nothing and raises nothing
    o = Owner.__new__(Owner)
    with pytest.raises(E.N_.MpeError):
        o.__init__(True)
    assert o.h is None
    o.close()
    o.__del__()
    assert Owner.destroyed == [1234]
    # __del__ alone closes, and swallows what a destroy raises
    o = Owner(False)
    o.__del__()
    assert Owner.destroyed == [1234, 1234] and o.h is None

    class Bad(E._Handle):
        h = 1

        def _destroy(self):
            raise RuntimeError("destroy failed")
    Bad().__del__()
    with pytest.raises(RuntimeError):
        Bad().close()


def test_every_owner_of_a_native_object_is_a_handle():
    from multi_party_ecdsa_amd import engine as E
    for name in HANDLE_OWNERS:
        cls = getattr(E, name)
        assert issubclass(cls, E._Handle) and cls.h is None, name
        assert "__del__" not in vars(cls), name                                        # the one __del__ is the base's
        assert ("_destroy" in vars(cls)) != (name == "Gg18Wallet"), name               # (the wallet owns two key sets, no handle)
        obj = cls.__new__(cls)                                                         # as after a constructor the library refused
        obj.close()
        obj.__del__()
    assert sorted(HANDLE_OWNERS) == sorted(c.__name__ for c in E._Handle.__subclasses__() if c.__module__ == E.__name__)


def test_typed_constants_come_from_the_header():
    from multi_party_ecdsa_amd import _abi, _native as N
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    try:
        import abi_model
    finally:
        sys.path.remove(os.path.join(ROOT, "tools"))
    model = dict(abi_model.constants())
    hdr = open(os.path.join(ROOT, "include", "mpecdsa_hip.h")).read()
    for short in TYPED:
        full = "MPE_" + short
        assert re.search(r"^#define\s+%s\s+\(\(\w+\)" % full, hdr, re.M), full         # it IS one of the typed ones
        assert full in model and getattr(N, short) == getattr(_abi, full) == model[full], full
    assert len(model) == len(re.findall(r"^#define\s+MPE_\w+\s", hdr, re.M))            # every object-like MPE_ macro is taken
    assert N.SEAL_MAGIC == int.from_bytes(b"MPS1", "little") and N.SEAL_KIND_USER == 16 and N.GG20_STATUS_BAD_TWEAK == 93
    text = open(os.path.join(ROOT, "multi_party_ecdsa_amd", "_native.py")).read()
    assert not re.search(r"^(?:SEAL|BIP32|SHA512|GG20)_\w+(?:, \w+)* = [\d(]", text, re.M)  # no number of its own
