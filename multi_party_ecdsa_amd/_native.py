"""ctypes binding of libmpecdsa_hip.so (the C-ABI declared in include/mpecdsa_hip.h).

The ABI is written in the header and nowhere else: _abi.py — the constants, the struct classes and the restype / argtypes of every
function — is generated from it by tools/gen_python_bindings.py (tests/test_abi_cpu.py refuses a stale copy and checks the struct
layouts against a C compiler).  This module adds what a header cannot say: where the library is, how an error is raised, the
dict form of `mpe_encoding`, and the short names engine.py and the tests use.

The HIP library is the product; there is no CPU fallback.  Importing this module without the
built shared object raises ImportError with the build command.
"""
import ctypes as C
import os

from . import _abi
from ._abi import *  # noqa: F401,F403  (MPE_* constants, the struct classes, SIGNATURES, EXPORTED)

_HERE = os.path.dirname(os.path.abspath(__file__))
# MPE_LIB_PATH: another build of the SAME library (A/B measurements of kernel variants, tools/ab.sh); never a different backend
LIB_PATH = os.environ.get("MPE_LIB_PATH") or os.path.join(_HERE, "libmpecdsa_hip.so")

# short names: MPE_GG20_STATUS_BAD_* -> GG20_STATUS_BAD_*, MPE_GG20_PRESIG_* -> PRESIG_*, mpe_gg20_blameN_in -> BlameNIn, and
# MPE_SEAL_* -> SEAL_*, MPE_GG20_KEYSHARE_WORDS, MPE_SHA512_* / MPE_BIP32_* of the sealed records and the child-key sessions
_SHORT = ("MPE_GG20_STATUS_", "MPE_GG20_KEYSHARE_", "MPE_SEAL_", "MPE_SHA512_", "MPE_BIP32_")
globals().update({k[len("MPE_"):]: v for k, v in vars(_abi).items() if k.startswith(_SHORT)})
globals().update({k[len("MPE_GG20_"):]: v for k, v in vars(_abi).items() if k.startswith("MPE_GG20_PRESIG_")})
Blame5In, Blame6In, Blame7In = _abi.Gg20Blame5In, _abi.Gg20Blame6In, _abi.Gg20Blame7In
GG20_NONCE_FIELDS = [f for f, _ in _abi.Gg20Nonces._fields_]
KEYGEN_ROUND1_FIELDS = [f for f, _ in _abi.KeygenRound1._fields_]


def gg20_status_pass_failed(rc):              # MPE_GG20_STATUS_PASS_FAILED(rc), a function-like macro of the header
    return 9000 - rc


class MpeError(RuntimeError):
    pass


class Encoding(_abi.Encoding):
    """`mpe_encoding` (include/mpecdsa_hip.h): the recalled byte-level conventions of curv / zk-paillier as a run-time profile"""
    SIZES = dict(ord_dlog=3, ord_pedersen=5, ord_heg=7, ord_ecddh=6, ord_cdlog=4)

    @classmethod
    def from_dict(cls, d):
        """d: {"chain_point": 0|1, "zero_bytes": 0|1, "ck_mask_order": 0|1, "ck_salt": int, "ord_*": [..]} (missing = default)"""
        e = cls()
        lib.mpe_encoding_default(C.byref(e))
        for k, v in d.items():
            if k.startswith("ord_"):
                arr = getattr(e, k)
                for i, x in enumerate(v):
                    arr[i] = x
            else:
                setattr(e, k, v)
        return e

    def as_dict(self):
        out = {k: getattr(self, k) for k in ("chain_point", "zero_bytes", "ck_mask_order", "ck_salt")}
        out.update({k: list(getattr(self, k))[:n] for k, n in self.SIZES.items()})
        return out


def _load():
    if not os.path.exists(LIB_PATH):
        raise ImportError(
            f"{LIB_PATH} is missing: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
            "(hipcc --offload-arch=gfx950). There is no CPU fallback for the HIP path.")
    lib = C.CDLL(LIB_PATH)
    for name, (res, args) in _abi.SIGNATURES.items():
        fn = getattr(lib, name)
        fn.restype = res
        fn.argtypes = args
    return lib


lib = _load()


def check(rc, what):
    if rc != _abi.MPE_OK:
        raise MpeError(f"{what} failed: rc={rc} ({lib.mpe_last_error().decode()})")


class _Call:
    """`call.mpe_X(*args)` is `check(lib.mpe_X(*args), "mpe_X")`: the function is named once.  `what=` replaces the name in the message.
    Only for functions that return a status: a count or a string (mpe_paillier_nkeys, mpe_last_error) is read through `lib`."""

    def __getattr__(self, name):
        if name not in _abi.SIGNATURES:
            raise AttributeError(f"{name} is not declared in include/mpecdsa_hip.h")
        if _abi.SIGNATURES[name][0] is not C.c_int:
            raise TypeError(f"{name} returns {_abi.SIGNATURES[name][0]}, not a status: call it through lib")
        fn = getattr(lib, name)

        def checked(*args, what=name):
            check(fn(*args), what)
        setattr(self, name, checked)              # looked up once per name
        return checked


call = _Call()
