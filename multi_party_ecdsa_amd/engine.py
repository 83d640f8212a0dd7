"""Thin object layer over the C-ABI: device buffers are torch tensors (int32 storage of the
u32 words), every compute call goes to libmpecdsa_hip.so.  Mirrors curv's `BigInt::mod_pow` /
`mod_mul` in batched form."""
import ctypes as C
import os

import numpy as np
import torch

from . import _native as N_                  # (N is a Paillier modulus in this file)
from . import wire
from .words import ints_to_words, words_to_ints


def _dev_u32(arr_np, device):
    """np.uint32 [.., ..] -> torch int32 tensor on device holding the same bits."""
    return torch.from_numpy(arr_np.view(np.int32)).to(device)


def _to_np_u32(t):
    return t.detach().cpu().numpy().view(np.uint32)


def _new(ctx, *shape):
    """an uninitialised int32 tensor (u32 words) on the context's device: _new(ctx, B, 16), _new(ctx, L, B, 8), _new(ctx, B)"""
    return torch.empty(shape, dtype=torch.int32, device=ctx.device)


def _flags(ctx, B):
    return torch.empty((B,), dtype=torch.uint8, device=ctx.device)


def _ptr(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


def dev(ctx, vals, words):
    """Python ints -> device word tensor"""
    return _dev_u32(ints_to_words(vals, words), ctx.device)


def host(t):
    """device word tensor -> Python ints"""
    return words_to_ints(_to_np_u32(t))


def _on_ints(ctx, device_call, *cols, idx=None):
    """the Python-int form of a device call: cols = (ints, words) per operand; device_call(*word tensors, index tensor or None)
    gives the device result, which is read back as ints after a sync"""
    d_idx = None if idx is None else torch.tensor(idx, dtype=torch.int32, device=ctx.device)
    d_out = device_call(*[dev(ctx, vals, words) for vals, words in cols], d_idx)
    ctx.sync()
    return host(d_out)


class _Handle:
    """The owner of one native object: `h` is None until the constructor has it and after close(); a subclass states its destroy call."""
    h = None

    def _destroy(self):
        raise NotImplementedError

    def close(self):
        if self.h:
            self._destroy()
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


# The LIBRARY reads no environment variable (mpe_ctx_set_option is the only way to change an A/B switch).  This harness — tests,
# bench.py, tools/ — keeps the MPE_* variables of the earlier rounds' measurement scripts working by translating them into options
# when it creates a context: MPE_NO_PAR=1 -> ("no_par", "1"), MPE_WIDE_DIV=4 -> ("wide_div", "4"), MPE_GRID=full -> ("grid", "full").
_ENV_OPTIONS = ["no_fixed_base", "no_crt", "no_multiexp", "no_pair", "no_pown", "no_sliding", "no_par", "no_wide", "no_adaptive_lanes",
                "no_merge_xn", "no_merge_r1", "fb_window_bits", "window_bits", "wide_div", "xwide_div", "waves_per_cu", "grid", "fb_budget_mb",
                "fb_split", "gg20_trace", "sampler_max_attempts", "safe_pass_log", "no_elect", "no_primaries", "merge_r1_quarters",
                "no_r1_inversion_ahead", "no_r1_dlog_first", "no_prio", "no_pdl_ahead", "no_crt_n", "no_r5_self_crt"]


def options_from_env(env=None):
    env = os.environ if env is None else env
    out = {}
    for k in _ENV_OPTIONS:
        v = env.get("MPE_" + k.upper())
        if v is not None and v != "":
            out[k] = v
    if env.get("MPE_GRID_EQUAL"):
        out["grid"] = "equal"
    return out


class Context(_Handle):
    def __init__(self, device=0, encoding=None, options=None):
        """encoding: None (the defaults of include/mpecdsa_hip.h) or a dict / _native.Encoding — the profile of the recalled
        curv / zk-paillier byte conventions this context hashes with (mpe_ctx_set_encoding).
        options: {key: value} for mpe_ctx_set_option, applied on top of the harness's MPE_* environment translation."""
        if not torch.cuda.is_available():
            raise N_.MpeError("no GPU visible: the HIP path cannot run (there is no CPU fallback)")
        self.device = torch.device("cuda", device)
        h = C.c_void_p()
        N_.call.mpe_ctx_create(C.byref(h), device)
        self.h = h
        if encoding is not None:
            self.set_encoding(encoding)
        self.options = {}
        for k, v in {**options_from_env(), **(options or {})}.items():
            self.set_option(k, v)

    def set_option(self, key, value):
        """mpe_ctx_set_option: an A/B switch of the measurements (none changes a result); before the dependent objects are created"""
        N_.call.mpe_ctx_set_option(self.h, str(key).encode(), str(int(value) if isinstance(value, bool) else value).encode(), what=f"mpe_ctx_set_option({key})")
        self.options[key] = value

    def get_option(self, key):
        v = C.c_long(0)
        N_.call.mpe_ctx_get_option(self.h, str(key).encode(), C.byref(v), what=f"mpe_ctx_get_option({key})")
        return v.value

    def set_device_share(self, contexts):
        """this many contexts work on the device at the same time (mpe_ctx_set_device_share): keep the efficient lane layouts"""
        N_.call.mpe_ctx_set_device_share(self.h, int(contexts))

    def set_encoding(self, encoding):
        e = encoding if isinstance(encoding, N_.Encoding) else N_.Encoding.from_dict(dict(encoding))
        N_.call.mpe_ctx_set_encoding(self.h, C.byref(e))

    def encoding(self):
        e = N_.Encoding()
        N_.call.mpe_ctx_get_encoding(self.h, C.byref(e))
        return e.as_dict()

    def stream(self):
        return C.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)

    def sync(self):
        N_.call.mpe_sync(self.h, self.stream())

    def launch_info(self):
        li = N_.LaunchInfo()
        N_.call.mpe_last_launch_info(self.h, C.byref(li))
        return {k: getattr(li, k) for k, _ in li._fields_}

    def prof_enable(self, on=True):
        N_.call.mpe_prof_enable(self.h, int(on))

    def prof_collect(self, max_records=4096):
        arr = (N_.ProfRec * max_records)()
        n = C.c_int(0)
        N_.call.mpe_prof_collect(self.h, arr, max_records, C.byref(n))
        return [dict(kind=r.kind, bits=r.bits, exp_words=r.exp_words, batch=r.batch, ms=r.ms, exp2_words=r.exp2_words,
                     sliding_frac=r.sliding_frac) for r in arr[:n.value]]

    def wipe(self):
        N_.call.mpe_ctx_wipe(self.h, self.stream())

    def scratch_audit(self):
        """(non-zero 32-bit words, total bytes) over every scratch region the context owns"""
        nz, tot = C.c_uint64(0), C.c_uint64(0)
        N_.call.mpe_ctx_scratch_audit(self.h, C.byref(nz), C.byref(tot), self.stream())
        return nz.value, tot.value

    def _destroy(self):
        N_.lib.mpe_ctx_destroy(self.h)


class ModSet(_Handle):
    """A set of odd moduli resident in HBM with their Montgomery constants (computed on the GPU)."""

    def __init__(self, ctx, bits, moduli):
        """moduli: list of ints, or a device int32 tensor [count, bits/32] of u32 words."""
        self.ctx, self.bits, self.k32 = ctx, bits, bits // 32
        if isinstance(moduli, torch.Tensor):
            self.d_moduli = moduli.contiguous()
        else:
            self.d_moduli = dev(ctx, moduli, self.k32)
        self.count = self.d_moduli.shape[0]
        h = C.c_void_p()
        N_.call.mpe_modset_create(ctx.h, bits, self.count, _ptr(self.d_moduli), C.byref(h), ctx.stream())
        self.h = h

    def _destroy(self):
        N_.lib.mpe_modset_destroy(self.h)


def modexp_device(ctx, ms, d_base, d_exp, d_out=None, d_mod_idx=None):
    """All-device call: d_base [B,k32], d_exp [B,ew], optional d_mod_idx [B] int32 -> d_out [B,k32]."""
    if d_out is None:
        d_out = torch.empty_like(d_base)
    N_.call.mpe_modexp(ctx.h, ms.h, d_base.shape[0], _ptr(d_mod_idx), _ptr(d_base), _ptr(d_exp), d_exp.shape[1], _ptr(d_out), ctx.stream())
    return d_out


def modmul_device(ctx, ms, d_a, d_b, d_out=None, d_mod_idx=None):
    if d_out is None:
        d_out = torch.empty_like(d_a)
    N_.call.mpe_modmul(ctx.h, ms.h, d_a.shape[0],_ptr(d_mod_idx), _ptr(d_a), _ptr(d_b), _ptr(d_out), ctx.stream())
    return d_out


def mod_pow2(ctx, ms, bases, exps, bases2, exps2, mod_idx=None, exp_bits=None, exp2_bits=None):
    """Batched `mod_pow(b, e, n) * mod_pow(b2, e2, n) % n` on one ladder (`mpe_modexp2`); e2 is the short exponent."""
    ew = ((exp_bits or max(1, max(int(e).bit_length() for e in exps))) + 31) // 32
    ew2 = ((exp2_bits or max(1, max(int(e).bit_length() for e in exps2))) + 31) // 32

    def modexp2_device(d_b, d_e, d_b2, d_e2, d_idx):
        d_out = torch.empty_like(d_b)
        N_.call.mpe_modexp2(ctx.h, ms.h, len(bases), _ptr(d_idx), _ptr(d_b), _ptr(d_e), ew, _ptr(d_b2), _ptr(d_e2), ew2, _ptr(d_out), ctx.stream())
        return d_out
    return _on_ints(ctx, modexp2_device, (bases, ms.k32), (exps, ew), (bases2, ms.k32), (exps2, ew2), idx=mod_idx)


def mod_pow(ctx, ms, bases, exps, mod_idx=None, exp_bits=None):
    """Batched `BigInt::mod_pow(base, exp, modulus)` on Python ints (host convenience wrapper)."""
    if exp_bits is None:
        exp_bits = max(1, max(int(e).bit_length() for e in exps))
    return _on_ints(ctx, lambda d_base, d_exp, d_idx: modexp_device(ctx, ms, d_base, d_exp, d_mod_idx=d_idx),
                    (bases, ms.k32), (exps, (exp_bits + 31) // 32), idx=mod_idx)


def mod_mul(ctx, ms, a, b, mod_idx=None):
    return _on_ints(ctx, lambda d_a, d_b, d_idx: modmul_device(ctx, ms, d_a, d_b, d_mod_idx=d_idx), (a, ms.k32), (b, ms.k32), idx=mod_idx)


class PaillierKeys(_Handle):
    """A set of Paillier-2048 keys in HBM (`EncryptionKey{n,nn}` / `DecryptionKey{p,q}` of kzen-paillier).
    Build from moduli (public) or from primes (private; enables decrypt)."""

    def __init__(self, ctx, N=None, p=None, q=None):
        self.ctx = ctx
        h = C.c_void_p()
        if p is not None:
            # Python ints, or device word tensors [nkeys, 32] (what paillier_keygen returns)
            self.d_p = p if torch.is_tensor(p) else dev(ctx, p, 32)
            self.d_q = q if torch.is_tensor(q) else dev(ctx, q, 32)
            N_.call.mpe_paillier_create_private(ctx.h, len(p), _ptr(self.d_p), _ptr(self.d_q), C.byref(h), ctx.stream())
            self.private = True
        else:
            self.d_N = dev(ctx, N, 64)
            N_.call.mpe_paillier_create_public(ctx.h, len(N), _ptr(self.d_N), C.byref(h), ctx.stream())
            self.private = False
        self.h = h
        self.nkeys = N_.lib.mpe_paillier_nkeys(h)

    def _destroy(self):
        N_.lib.mpe_paillier_destroy(self.h)

    # ---- device-tensor API (int32 tensors holding u32 words) ----
    def encrypt_device(self, d_m, d_r, d_key_idx=None, d_c=None):
        """`Paillier::encrypt_with_chosen_randomness` batched: m,r [B,64] -> c [B,128]"""
        B = d_m.shape[0]
        if d_c is None:
            d_c = torch.empty((B, 128), dtype=torch.int32, device=d_m.device)
        N_.call.mpe_paillier_encrypt(self.ctx.h, self.h, B, _ptr(d_key_idx), _ptr(d_m), _ptr(d_r), _ptr(d_c), self.ctx.stream())
        return d_c

    def decrypt_device(self, d_c, d_key_idx=None, d_m=None):
        """`Paillier::decrypt` batched: c [B,128] -> m [B,64]"""
        B = d_c.shape[0]
        if d_m is None:
            d_m = torch.empty((B, 64), dtype=torch.int32, device=d_c.device)
        N_.call.mpe_paillier_decrypt(self.ctx.h, self.h, B, _ptr(d_key_idx), _ptr(d_c), _ptr(d_m), self.ctx.stream())
        return d_m

    def add_device(self, d_c1, d_c2, d_key_idx=None):
        out = torch.empty_like(d_c1)
        N_.call.mpe_paillier_add(self.ctx.h, self.h, d_c1.shape[0], _ptr(d_key_idx), _ptr(d_c1), _ptr(d_c2), _ptr(out), self.ctx.stream())
        return out

    def mul_device(self, d_c, d_k, d_key_idx=None):
        out = torch.empty_like(d_c)
        N_.call.mpe_paillier_mul(self.ctx.h, self.h, d_c.shape[0], _ptr(d_key_idx), _ptr(d_c), _ptr(d_k), d_k.shape[1], _ptr(out), self.ctx.stream())
        return out

    # ---- Python-int convenience wrappers ----
    def encrypt(self, m, r, key_idx=None):
        return _on_ints(self.ctx, self.encrypt_device, (m, 64), (r, 64), idx=key_idx)

    def decrypt(self, c, key_idx=None):
        return _on_ints(self.ctx, self.decrypt_device, (c, 128), idx=key_idx)

    def add(self, c1, c2, key_idx=None):
        return _on_ints(self.ctx, self.add_device, (c1, 128), (c2, 128), idx=key_idx)

    def mul(self, c, k, key_idx=None, k_words=8):
        return _on_ints(self.ctx, self.mul_device, (c, 128), (k, k_words), idx=key_idx)


# ================================================================================================
# secp256k1, modinv, DLogStatement tables and the proofs (device-tensor API; int32 tensors of u32 words)
# ================================================================================================
def modinv_device(ctx, ms, d_a, d_mod_idx=None):
    B = d_a.shape[0]
    out, ok = torch.empty_like(d_a), _flags(ctx, B)
    N_.call.mpe_modinv(ctx.h, ms.h, B, _ptr(d_mod_idx), _ptr(d_a), _ptr(out), _ptr(ok), ctx.stream())
    return out, ok


def ec_mul_base(ctx, d_k):
    out = _new(ctx, d_k.shape[0], 16)
    N_.call.mpe_ec_mul_base(ctx.h, d_k.shape[0], _ptr(d_k), d_k.shape[1], _ptr(out), ctx.stream())
    return out


def ec_mul(ctx, d_k, d_P):
    out = _new(ctx, d_k.shape[0], 16)
    N_.call.mpe_ec_mul(ctx.h, d_k.shape[0], _ptr(d_k), d_k.shape[1], _ptr(d_P), _ptr(out), ctx.stream())
    return out


def ec_add(ctx, d_P, d_Q):
    out = _new(ctx, d_P.shape[0], 16)
    N_.call.mpe_ec_add(ctx.h, d_P.shape[0], _ptr(d_P), _ptr(d_Q), _ptr(out), ctx.stream())
    return out


def dlog_prove(ctx, d_sk, d_nonce):
    B = d_sk.shape[0]
    pk, R, z = _new(ctx, B, 16), _new(ctx, B, 16), _new(ctx, B, 8)
    N_.call.mpe_dlog_prove(ctx.h, B, _ptr(d_sk), _ptr(d_nonce), _ptr(pk), _ptr(R), _ptr(z), ctx.stream())
    return pk, R, z


def dlog_verify(ctx, d_pk, d_R, d_z):
    ok = _flags(ctx, d_pk.shape[0])
    N_.call.mpe_dlog_verify(ctx.h, d_pk.shape[0], _ptr(d_pk), _ptr(d_R), _ptr(d_z), _ptr(ok), ctx.stream())
    return ok


class Statements(_Handle):
    """Table of `DLogStatement{N: N~, g: h1, ni: h2}` (party_i.rs:225-229) resident in HBM."""

    def __init__(self, ctx, Nt, h1, h2, wb=None):
        """wb: None = the context's window width of the fixed-base tables; 0 = one-off statements without tables (mpe_statements_create_wb)"""
        self.ctx = ctx
        self.d = [v if torch.is_tensor(v) else dev(ctx, v, 64) for v in (Nt, h1, h2)]      # ints, or device word tensors [count, 64]
        h = C.c_void_p()
        if wb is None:
            N_.call.mpe_statements_create(ctx.h, len(Nt), _ptr(self.d[0]), _ptr(self.d[1]), _ptr(self.d[2]), C.byref(h), ctx.stream())
        else:
            N_.call.mpe_statements_create_wb(ctx.h, len(Nt), _ptr(self.d[0]), _ptr(self.d[1]), _ptr(self.d[2]), int(wb), C.byref(h), ctx.stream())
        self.h, self.count = h, len(Nt)

    def _destroy(self):
        N_.lib.mpe_statements_destroy(self.h)


ALICE_PROOF_WORDS = dict(z=64, e=8, s=64, s1=25, s2=89)
ALICE_NONCE_WORDS = dict(alpha=24, beta=64, gamma=88, rho=72)
PDL_PROOF_WORDS = dict(z=64, u1=16, u2=128, u3=64, s1=25, s2=64, s3=89)
PDL_NONCE_WORDS = dict(alpha=24, beta=64, rho=72, gamma=88)


def _struct(cls, tensors):
    s = cls()
    for f, _ in cls._fields_:
        setattr(s, f, tensors[f].data_ptr())
    return s


def alice_generate(ctx, pk, stm, d_a, d_cipher, d_r, nonces, d_key_idx=None, d_st_idx=None):
    """`AliceProof::generate` batched.  nonces / result: dict of device tensors (widths: ALICE_*_WORDS)."""
    B = d_a.shape[0]
    out = {f: _new(ctx, B, w) for f, w in ALICE_PROOF_WORDS.items()}
    nn, pr = _struct(N_.AliceNonces, nonces), _struct(N_.AliceProof, out)
    N_.call.mpe_alice_generate(ctx.h, pk.h, stm.h, B, _ptr(d_key_idx), _ptr(d_st_idx), _ptr(d_a), _ptr(d_cipher), _ptr(d_r), C.byref(nn), C.byref(pr),
                               ctx.stream())
    return out


def alice_verify(ctx, pk, stm, d_cipher, proof, d_key_idx=None, d_st_idx=None):
    B = d_cipher.shape[0]
    ok = _flags(ctx, B)
    pr = _struct(N_.AliceProof, proof)
    N_.call.mpe_alice_verify(ctx.h, pk.h, stm.h, B, _ptr(d_key_idx), _ptr(d_st_idx), _ptr(d_cipher), C.byref(pr), _ptr(ok), ctx.stream())
    return ok


def pdl_prove(ctx, pk, stm, d_cipher, d_Q, d_G, d_x, d_r, nonces, d_key_idx=None, d_st_idx=None):
    """`PDLwSlackProof::prove` batched."""
    B = d_x.shape[0]
    out = {f: _new(ctx, B, w) for f, w in PDL_PROOF_WORDS.items()}
    nn, pr = _struct(N_.PdlNonces, nonces), _struct(N_.PdlProof, out)
    N_.call.mpe_pdl_prove(ctx.h, pk.h, stm.h, B, _ptr(d_key_idx), _ptr(d_st_idx), _ptr(d_cipher), _ptr(d_Q), _ptr(d_G), _ptr(d_x), _ptr(d_r), C.byref(nn),
                          C.byref(pr), ctx.stream())
    return out


def pdl_verify(ctx, pk, stm, d_cipher, d_Q, d_G, proof, d_key_idx=None, d_st_idx=None):
    B = d_cipher.shape[0]
    ok = _flags(ctx, B)
    pr = _struct(N_.PdlProof, proof)
    N_.call.mpe_pdl_verify(ctx.h, pk.h, stm.h, B, _ptr(d_key_idx), _ptr(d_st_idx), _ptr(d_cipher), _ptr(d_Q), _ptr(d_G), C.byref(pr), _ptr(ok), ctx.stream())
    return ok


# ================================================================================================
# GG20 signing: key object, the per-party round view, the lock-step composition
# ================================================================================================
GG20_ROUNDS = [0, 1, 2, 3, 4, 5, 7]             # rounds that emit a message


def gg20_msg_words(S, n, rnd):
    return N_.lib.mpe_gg20_msg_words(S, n, rnd)


class Gg20Keys(_Handle):
    """`LocalKey` material (keygen/rounds.rs:311-322) + the signer set, resident in HBM.
    arrays: dict of numpy uint32 arrays for ALL n parties of every key set: x [K*n,8], p, q [K*n,32], Nt, h1, h2 [K*n,64],
    y [K,16], X [K*n,16] (and optionally N [K*n,64], else p*q).  own: the party indices whose SECRETS (x, p, q) this
    object gets (default: all — the Simulation harness); the other parties' rows of x, p, q never leave the host.
    signer_sets=[[...], ...] (instead of `signers`): one object that signs for several quorums of the wallet
    (mpe_gg20_keys_create_sets); a session names its set by its index in this list (`sigset=`), set 0 where none is named.
    sealed_shares, wrap: the secrets as sealed key shares [K*n, 82] (numpy uint32 or device int32, what gg20_keygen(..., wrap=) returns)
    under the WrapKey `wrap`, instead of x, p, q in `arrays` (which then needs N): they are unsealed on the device
    (mpe_gg20_keys_create_sealed) and no clear secret passes through the host."""

    def __init__(self, ctx, t, n, signers, arrays, own=None, nkeysets=1, signer_sets=None, sealed_shares=None, wrap=None):
        if (sealed_shares is None) != (wrap is None):
            raise ValueError("Gg20Keys: sealed_shares and wrap go together")
        if signer_sets is None:
            signer_sets = [list(signers)]
        elif signers is not None and [int(x) for x in signers] != [int(x) for x in signer_sets[0]]:
            raise ValueError("Gg20Keys: `signers` is set 0 of `signer_sets`")
        self.signer_sets = [[int(x) for x in s] for s in signer_sets]
        signers = self.signer_sets[0]
        self.ctx, self.t, self.n, self.S, self.K = ctx, t, n, len(signers), nkeysets
        own = list(range(n)) if own is None else sorted(int(a) for a in own)
        self.own = own
        sealed = sealed_shares is not None
        a = {f: np.ascontiguousarray(arrays[f]) for f in (() if sealed else ("x", "p", "q")) + ("Nt", "h1", "h2", "y", "X")}
        if "N" in arrays and arrays["N"] is not None:
            a["N"] = np.ascontiguousarray(arrays["N"])
        elif sealed:
            raise ValueError("Gg20Keys: sealed shares need arrays['N']")
        else:
            ps, qs = words_to_ints(a["p"]), words_to_ints(a["q"])
            a["N"] = ints_to_words([p_ * q_ for p_, q_ in zip(ps, qs)], 64)
        rows = [kk * n + o for kk in range(nkeysets) for o in own]
        h = {f: a[f] for f in ("N", "Nt", "h1", "h2", "y", "X")}
        for f in (() if sealed else ("x", "p", "q")):
            h[f] = np.ascontiguousarray(a[f][rows])
        self.d = {f: torch.from_numpy(h[f].view(np.int32)).to(ctx.device) for f in h}
        if sealed:
            sh = sealed_shares if torch.is_tensor(sealed_shares) else torch.from_numpy(np.ascontiguousarray(sealed_shares).view(np.int32))
            self.d["sealed"] = sh.to(ctx.device)[torch.tensor(rows, device=ctx.device)].contiguous()
        ow = (C.c_int32 * len(own))(*own)
        hd = C.c_void_p()
        pub = [_ptr(self.d[f]) for f in ("N", "Nt", "h1", "h2", "y", "X")]
        dev = ([wrap.h, _ptr(self.d["sealed"])] if sealed else [_ptr(self.d[f]) for f in ("x", "p", "q")]) + pub
        if sealed:
            flat = [x for s in self.signer_sets for x in s]
            sg = (C.c_int32 * len(flat))(*flat)
            if len(flat) != len(self.signer_sets) * self.S:
                raise ValueError("every signer set of a key object has the same number of signers")
            N_.call.mpe_gg20_keys_create_sealed(ctx.h, t, n, self.S, len(self.signer_sets), sg, nkeysets, len(own), ow, *dev, C.byref(hd), ctx.stream())
        elif len(self.signer_sets) == 1:
            sg = (C.c_int32 * len(signers))(*signers)
            N_.call.mpe_gg20_keys_create(ctx.h, t, n, len(signers), sg, nkeysets, len(own), ow, *dev, C.byref(hd), ctx.stream())
        else:
            flat = [x for s in self.signer_sets for x in s]      # (the library checks the rows: its refusals are part of its contract)
            sg = (C.c_int32 * len(flat))(*flat)
            if len(flat) != len(self.signer_sets) * self.S:
                raise ValueError("every signer set of a key object has the same number of signers")
            N_.call.mpe_gg20_keys_create_sets(ctx.h, t, n, self.S, len(self.signer_sets), sg, nkeysets, len(own), ow, *dev, C.byref(hd), ctx.stream())
        self.h = hd

    def fb_window_bits(self):
        return N_.lib.mpe_gg20_keys_fb_window_bits(self.h)

    def _destroy(self):
        N_.lib.mpe_gg20_keys_destroy(self.h)


class Gg20Session(_Handle):
    """`RoundN::proceed` for B sessions x the local parties `local` (signer ordinals).  nonces: dict of device int32
    tensors with leading dimensions [B][len(local)] (fields _native.GG20_NONCE_FIELDS; `msg` optional).
    sigset: device int32 [B], the signer set (index into keys.signer_sets) of every session; ordinals are then positions in each
    session's own set.  local_party=p (instead of `local`): the one local party by its party INDEX, its ordinal in a session is its
    rank in that session's set (mpe_gg20_session_create_sets).
    tweaks: device int32 [B, 8], the public tweak of every session (E.bip32_derive): session b signs for the child key x + t_b
    (mpe_gg20_session_create_tweaks); child_keys() gives the public keys."""

    def __init__(self, ctx, keys, B, local, nonces, keyset=None, dedup_verify=False, sigset=None, local_party=None, tweaks=None):
        by_party = local_party is not None
        if by_party:
            local = [int(local_party)] if local is None else list(local)
        self.ctx, self.keys, self.B, self.local = ctx, keys, B, [int(x) for x in local]
        self.S, self.n, self.L = keys.S, keys.n, len(local)
        self._sigset = sigset
        self._nonces = dict(nonces)
        if "msg" not in self._nonces:
            self._nonces["msg"] = torch.zeros((B, 8), dtype=torch.int32, device=ctx.device)
        self._keyset = keyset
        nn = _struct(N_.Gg20Nonces, self._nonces)
        lc = (C.c_int32 * self.L)(*self.local)
        h = C.c_void_p()
        if tweaks is not None:
            tweaks = tweaks.contiguous()
            N_.call.mpe_gg20_session_create_tweaks(ctx.h, keys.h, B, self.L, lc, _ptr(keyset), _ptr(sigset), int(by_party), _ptr(tweaks), C.byref(nn),
                                                   int(bool(dedup_verify)), C.byref(h), ctx.stream())
        elif sigset is None and not by_party:
            N_.call.mpe_gg20_session_create(ctx.h, keys.h, B, self.L, lc, _ptr(keyset), C.byref(nn), int(bool(dedup_verify)), C.byref(h), ctx.stream())
        else:
            N_.call.mpe_gg20_session_create_sets(ctx.h, keys.h, B, self.L, lc, _ptr(keyset), _ptr(sigset), int(by_party), C.byref(nn), int(bool(dedup_verify)),
                                                 C.byref(h), ctx.stream())
        self.h = h

    def _off(self, in_off):
        return None if in_off is None else (C.c_int64 * self.S)(*[int(x) for x in in_off])

    def rearm(self, nonces, keyset=None, sigset=None, tweaks=None):
        """the next batch of the same shape on this object (mpe_gg20_session_rearm[_sets | _tweaks]): fresh sampled values, rounds from 0"""
        self._nonces = dict(nonces)
        if "msg" not in self._nonces:
            self._nonces["msg"] = torch.zeros((self.B, 8), dtype=torch.int32, device=self.ctx.device)
        self._keyset = keyset
        nn = _struct(N_.Gg20Nonces, self._nonces)
        self._sigset = sigset
        if tweaks is not None:
            N_.call.mpe_gg20_session_rearm_tweaks(self.h, _ptr(keyset), _ptr(sigset), _ptr(tweaks.contiguous()), C.byref(nn), self.ctx.stream())
        elif sigset is None:
            N_.call.mpe_gg20_session_rearm(self.h, _ptr(keyset), C.byref(nn), self.ctx.stream())
        else:
            N_.call.mpe_gg20_session_rearm_sets(self.h, _ptr(keyset), _ptr(sigset), C.byref(nn), self.ctx.stream())

    def child_keys(self):
        """[B, 16] device int32: the public key every session of the batch signs for (mpe_gg20_session_child_keys)"""
        y = _new(self.ctx, self.B, 16)
        N_.call.mpe_gg20_session_child_keys(self.h, _ptr(y), self.ctx.stream())
        return y

    def abort(self):
        """mpe_gg20_session_abort: give the running batch up (state wiped now); rearm() starts the next one"""
        N_.call.mpe_gg20_session_abort(self.h, self.ctx.stream())

    def round(self, rnd, d_in=None, in_off=None, msg=None, out=None):
        """Runs round `rnd` (0..7, 8 = SignManual::complete).  d_in: the previous round's records of all S senders (device
        int32 tensor; sender j's [B][W] block at record in_off[j], default j*B).  Returns this object's outgoing records
        [L, B, W] (None for rounds 6 and 8); `out`: a contiguous [L, B, W] int32 device tensor to write them into (e.g. this
        rank's slot of an all-gather buffer)."""
        st = self.ctx.stream()
        W = gg20_msg_words(self.S, self.n, rnd) if rnd in GG20_ROUNDS else 0
        if out is not None and W:
            if not (out.is_contiguous() and out.dtype == torch.int32 and out.numel() == self.L * self.B * W and out.device == self.ctx.device):
                raise ValueError("round(out=...): need a contiguous int32 [L, B, W] tensor on the context's device")
        else:
            out = _new(self.ctx, self.L, self.B, W) if W else None
        if rnd == 0:
            N_.call.mpe_gg20_round0(self.h, _ptr(out), st)
        elif 1 <= rnd <= 5:
            getattr(N_.call, f"mpe_gg20_round{rnd}")(self.h, _ptr(d_in), self._off(in_off), _ptr(out), st)
        elif rnd == 6:
            N_.call.mpe_gg20_round6(self.h, _ptr(d_in), self._off(in_off), st)
        elif rnd == 7:
            N_.call.mpe_gg20_round7(self.h, _ptr(msg), _ptr(out), st)
        elif rnd == 8:
            N_.call.mpe_gg20_complete(self.h, _ptr(d_in), self._off(in_off), st)
        else:
            raise ValueError(rnd)
        return out

    def fault_inject(self, step, party_mask):
        N_.call.mpe_gg20_session_fault_inject(self.h, int(step), int(party_mask))

    def blame6_state(self, d_nonce):
        """(miu [L,B,S-1,64], a1, a2 [L,B,16], z [L,B,8]): what the local parties publish for the phase-6 blame"""
        ctx, L, B = self.ctx, self.L, self.B
        miu, a1, a2, z = _new(ctx, L, B, self.S - 1, 64), _new(ctx, L, B, 16), _new(ctx, L, B, 16), _new(ctx, L, B, 8)
        N_.call.mpe_gg20_session_blame6_state(self.h, _ptr(d_nonce), _ptr(miu), _ptr(a1), _ptr(a2), _ptr(z), self.ctx.stream())
        return miu, a1, a2, z

    def result(self, signature=True):
        """dict of device tensors: status, bad_actors, recid [L,B]; r, s [L,B,8]; R [L,B,16]"""
        ctx, L, B = self.ctx, self.L, self.B
        o = dict(status=_new(ctx, L, B), bad_actors=_new(ctx, L, B), R=_new(ctx, L, B, 16))
        if signature:
            o.update(r=_new(ctx, L, B, 8), s=_new(ctx, L, B, 8), recid=_new(ctx, L, B))
        N_.call.mpe_gg20_session_result(self.h, _ptr(o["status"]), _ptr(o["bad_actors"]), _ptr(o.get("r")), _ptr(o.get("s")), _ptr(o.get("recid")),
                                        _ptr(o["R"]), self.ctx.stream())
        return o

    def _destroy(self):
        N_.lib.mpe_gg20_session_destroy(self.h, self.ctx.stream())


def gg20_sign(ctx, keys, nonces, B, dedup_verify=False, chunk=0, want_R=False, keyset=None, sigset=None, tweaks=None):
    """nonces: dict of device int32 tensors (fields _native.GG20_NONCE_FIELDS, [B][S] layout).  Returns device tensors
    r [B,8], s [B,8], recid [B], status [B] (0 = signed and verified) and optionally R [B,16].  sigset: device int32 [B], the signer
    set of every session (mpe_gg20_sign_sets).  tweaks: device int32 [B, 8], session b signs for the child key x + t_b
    (mpe_gg20_sign_tweaks)."""
    r, s, recid = _new(ctx, B, 8), _new(ctx, B, 8), _new(ctx, B)
    status = torch.full((B,), -1, dtype=torch.int32, device=ctx.device)
    R = _new(ctx, B, 16) if want_R else None
    nn = _struct(N_.Gg20Nonces, nonces)
    if tweaks is not None:
        N_.call.mpe_gg20_sign_tweaks(ctx.h, keys.h, B, _ptr(keyset), _ptr(sigset), _ptr(tweaks.contiguous()), C.byref(nn), _ptr(r), _ptr(s), _ptr(recid),
                                     _ptr(R), _ptr(status), int(bool(dedup_verify)), int(chunk), ctx.stream())
    elif sigset is None:
        N_.call.mpe_gg20_sign(ctx.h, keys.h, B, _ptr(keyset), C.byref(nn), _ptr(r), _ptr(s), _ptr(recid), _ptr(R), _ptr(status), int(bool(dedup_verify)),
                              int(chunk), ctx.stream())
    else:
        N_.call.mpe_gg20_sign_sets(ctx.h, keys.h, B, _ptr(keyset), _ptr(sigset), C.byref(nn), _ptr(r), _ptr(s), _ptr(recid), _ptr(R), _ptr(status),
                                   int(bool(dedup_verify)), int(chunk), ctx.stream())
    return (r, s, recid, status, R) if want_R else (r, s, recid, status)


class WrapKey(_Handle):
    """A wrapping key for sealed records (`mpe_wrap_key`): 32 bytes from the operator's KMS or HSM, copied into device memory the
    object owns and zeroed there when it is closed.  Every sealing call needs a `nonce_hi` that is never used twice with this key:
    unless one is given, 64 fresh random bits (`secrets.randbits`) per call."""

    def __init__(self, ctx, key_bytes):
        key_bytes = bytes(key_bytes)
        if len(key_bytes) != 32:
            raise ValueError("WrapKey: 32 bytes")
        self.ctx = ctx
        h = C.c_void_p()
        N_.call.mpe_wrap_key_create(ctx.h, key_bytes, C.byref(h))
        self.h = h

    @staticmethod
    def nonce(nonce_hi=None):
        import secrets
        return C.c_uint64(secrets.randbits(64) if nonce_hi is None else int(nonce_hi))

    def _destroy(self):
        N_.lib.mpe_wrap_key_destroy(self.h)


def seal(ctx, wrap, kind, d_plain, nonce_hi=None):
    """caller rows (kind >= 16): d_plain [count, words] device int32 -> sealed rows [count, words + 10] (mpe_seal)"""
    d_plain = d_plain.contiguous()
    count, words = d_plain.shape
    out = _new(ctx, count, words + 10)
    N_.call.mpe_seal(ctx.h, wrap.h, int(kind), count, words, _ptr(d_plain), WrapKey.nonce(nonce_hi), _ptr(out), ctx.stream())
    return out


def unseal(ctx, wrap, kind, d_sealed):
    """sealed rows [count, words + 10] -> (plain [count, words], status [count]): 841 and an all-zero row where a row is refused"""
    d_sealed = d_sealed.contiguous()
    count, words = d_sealed.shape[0], d_sealed.shape[1] - 10
    plain, status = _new(ctx, count, words), _new(ctx, count)
    N_.call.mpe_unseal(ctx.h, wrap.h, int(kind), count, words, _ptr(d_sealed), _ptr(plain), _ptr(status), ctx.stream())
    return plain, status


def poly1305(ctx, d_key, d_msg):
    """the one-time-key MAC on its own: d_key [count, 8] int32 (r | s), d_msg [count, bytes] uint8 -> tags [count, 4] int32"""
    d_key, d_msg = d_key.contiguous(), d_msg.contiguous()
    count = d_key.shape[0]
    tag = _new(ctx, count, 4)
    N_.call.mpe_poly1305(ctx.h, count, _ptr(d_key), _ptr(d_msg), d_msg.shape[1], _ptr(tag), ctx.stream())
    return tag


def _bytes_rows(ctx, rows, name):
    """device uint8 [count, bytes] of a tensor, or of a list of equally long bytes objects"""
    if isinstance(rows, torch.Tensor):
        if rows.dtype != torch.uint8 or rows.dim() != 2:
            raise ValueError(f"{name}: a uint8 [count, bytes] tensor")
        return rows.to(ctx.device).contiguous()
    rows = [bytes(r) for r in rows]
    if len({len(r) for r in rows}) > 1:
        raise ValueError(f"{name}: rows of one length")
    return torch.tensor([list(r) for r in rows], dtype=torch.uint8, device=ctx.device).reshape(len(rows), len(rows[0]) if rows else 0)


def sha512(ctx, msg):
    """msg: uint8 [count, bytes] (device tensor, or a list of bytes of one length, at most _native.SHA512_MAX_MSG_BYTES)
    -> digests, device uint8 [count, 64] (mpe_sha512)"""
    d_msg = _bytes_rows(ctx, msg, "sha512")
    out = torch.empty((d_msg.shape[0], 64), dtype=torch.uint8, device=ctx.device)
    N_.call.mpe_sha512(ctx.h, d_msg.shape[0], _ptr(d_msg), d_msg.shape[1], _ptr(out), ctx.stream())
    return out


def hmac_sha512(ctx, key, msg):
    """key: uint8 [count, 0..128], msg: uint8 [count, bytes] -> device uint8 [count, 64] (mpe_hmac_sha512)"""
    d_key, d_msg = _bytes_rows(ctx, key, "hmac_sha512 key"), _bytes_rows(ctx, msg, "hmac_sha512 msg")
    if d_key.shape[0] != d_msg.shape[0]:
        raise ValueError("hmac_sha512: one key per message")
    out = torch.empty((d_msg.shape[0], 64), dtype=torch.uint8, device=ctx.device)
    N_.call.mpe_hmac_sha512(ctx.h, d_msg.shape[0], _ptr(d_key), d_key.shape[1], _ptr(d_msg), d_msg.shape[1], _ptr(out), ctx.stream())
    return out


def bip32_derive(ctx, d_pub, cc, paths, depth=None, parent_idx=None):
    """BIP32 CKDpub along non-hardened paths (mpe_bip32_derive).  d_pub: parents' public keys, device int32 [n_parents, 16] (or [16]);
    cc: their chain codes, uint8 [n_parents, 32] (tensor or list of bytes); paths: [B, max_depth] indices (tensor or nested list, values
    below 2^32); depth: [B] levels used of each row (default: all max_depth); parent_idx: [B] (default: parent 0).
    Returns device tensors (tweak int32 [B, 8], child_pub int32 [B, 16], child_cc uint8 [B, 32], status int32 [B]); a row whose status
    is not 0 has the all-ones tweak, which a session refuses."""
    dv = ctx.device
    d_pub = d_pub.reshape(-1, 16).contiguous()
    d_cc = _bytes_rows(ctx, [cc] if isinstance(cc, (bytes, bytearray)) else cc, "bip32_derive cc")
    if d_cc.shape != (d_pub.shape[0], 32):
        raise ValueError("bip32_derive: one 32-byte chain code per parent")
    if isinstance(paths, torch.Tensor):
        d_path = paths.to(dv).to(torch.int32).contiguous()
    else:
        d_path = torch.from_numpy(np.ascontiguousarray(np.array(paths, dtype=np.uint32).reshape(len(paths), -1)).view(np.int32)).to(dv)
    B, max_depth = d_path.shape
    i32 = lambda v, fill: (torch.full((B,), fill, dtype=torch.int32, device=dv) if v is None else
                           (v.to(dv).to(torch.int32).contiguous() if isinstance(v, torch.Tensor) else torch.tensor(list(v), dtype=torch.int32, device=dv)))
    d_depth = i32(depth, max_depth)
    d_pidx = None if parent_idx is None else i32(parent_idx, 0)
    tweak, child, status = _new(ctx, B, 8), _new(ctx, B, 16), _new(ctx, B)
    ccs = torch.empty((B, 32), dtype=torch.uint8, device=dv)
    N_.call.mpe_bip32_derive(ctx.h, B, d_pub.shape[0], _ptr(d_pub), _ptr(d_cc), _ptr(d_pidx), _ptr(d_path), _ptr(d_depth), max_depth, _ptr(tweak), _ptr(child),
                             _ptr(ccs), _ptr(status), ctx.stream())
    return tweak, child, ccs, status


def keyshare_seal(ctx, wrap, d_x, d_p, d_q, nonce_hi=None):
    """x [count, 8], p, q [count, 32] (device int32) -> sealed key shares [count, 82] (mpe_gg20_keyshare_seal)"""
    count = d_x.shape[0]
    d_x, d_p, d_q = d_x.contiguous(), d_p.contiguous(), d_q.contiguous()        # (held until the call is queued)
    out = _new(ctx, count, N_.GG20_KEYSHARE_WORDS + 10)
    N_.call.mpe_gg20_keyshare_seal(ctx.h, wrap.h, count, _ptr(d_x), _ptr(d_p), _ptr(d_q), WrapKey.nonce(nonce_hi), _ptr(out), ctx.stream())
    return out


class PresigPool(_Handle):
    """Device-resident presignatures in single-use slots (`mpe_gg20_presig_*`): `CompletedOfflineStage` of `capacity` sessions for the
    local parties `local` (signer ordinals), kept until the message arrives.  The C-ABI is mechanism only; this object owns the POLICY:
    a host-side free list that hands slots to `deposit` / `import_` and takes them back when a row failed, a signature completed, or
    the slots were exported or discarded.  Slot arguments are lists, numpy arrays or device int32 tensors."""
    STATES = ("EMPTY", "READY", "SIGNED", "BUSY")

    def __init__(self, ctx, keys, local, capacity):
        self.ctx, self.keys, self.local, self.capacity = ctx, keys, [int(x) for x in local], int(capacity)
        self.S, self.L = keys.S, len(self.local)
        lc = (C.c_int32 * self.L)(*self.local)
        h = C.c_void_p()
        N_.call.mpe_gg20_presig_pool_create(ctx.h, keys.h, self.L, lc, self.capacity, C.byref(h))
        self.h = h
        self.capacity = N_.lib.mpe_gg20_presig_pool_capacity(h)
        self.record_words = N_.lib.mpe_gg20_presig_record_words(h)
        self.sealed_words = N_.lib.mpe_gg20_sealed_presig_words(h)
        self._used = set()                       # slots the free list has handed out (or the caller named) and not got back
        self._pending = []                       # (slots, device status, rows-per-slot) of calls whose freed slots are not yet counted
        self.last_status = None                  # numpy row statuses of the last deposit / import_

    # ---- the free list -----------------------------------------------------------------------------------------------------
    def _slots(self, slots):
        if torch.is_tensor(slots):
            return slots.to(device=self.ctx.device, dtype=torch.int32).contiguous()
        return torch.from_numpy(np.ascontiguousarray(slots, dtype=np.int32)).to(self.ctx.device)

    def _reap(self):
        """takes back the slots that completed, exported or discarded rows have emptied"""
        for d_slot, d_status in self._pending:
            sl = d_slot.cpu().numpy()
            ok = np.ones(len(sl), dtype=bool) if d_status is None else (d_status.cpu().numpy().reshape(-1, len(sl)) < 800).all(axis=0)
            self._used.difference_update(int(x) for x in sl[ok])
        self._pending = []

    def free_slots(self):
        self._reap()
        return self.capacity - len(self._used)

    def _take(self, count):
        self._reap()
        out = [s for s in range(self.capacity) if s not in self._used][:count]
        if len(out) < count:
            raise N_.MpeError(f"presignature pool: {count} slots wanted, {len(out)} free")
        return out

    def _filled(self, slots, status, chosen_by_caller):
        """after deposit / import_: the rows that filled their slot keep it; returns the usable slots, -1 for the other rows"""
        self.last_status = status
        good = status == 0
        if chosen_by_caller:
            self._used.update(int(x) for x in np.asarray(slots)[good])
        else:
            self._used.difference_update(int(x) for x in np.asarray(slots)[~good])
        return np.where(good, np.asarray(slots, dtype=np.int32), -1).astype(np.int32)

    # ---- the calls ---------------------------------------------------------------------------------------------------------------
    def deposit(self, session, slots=None):
        """moves the presignatures of a session behind round 6 into free slots (or into `slots`, one per session row) and wipes the
        session, which then waits for rearm().  Returns the usable slots [B] (numpy int32; -1 where the row failed: last_status)."""
        mine = slots is None
        if mine:
            slots = self._take(session.B)
            self._used.update(slots)
        d_slot = self._slots(slots)
        if d_slot.numel() != session.B:
            raise ValueError("deposit: one slot per session row")
        d_status = _new(self.ctx, session.B)
        try:
            N_.call.mpe_gg20_presig_deposit(self.h, session.h, _ptr(d_slot), _ptr(d_status), self.ctx.stream())
        except N_.MpeError:
            if mine:
                self._used.difference_update(slots)
            raise
        return self._filled(d_slot.cpu().numpy(), d_status.cpu().numpy(), not mine)

    def sign(self, slots, msg):
        """`Round7::new` for READY slots: (s_i [L, count, 8], status [count]) device tensors; msg [count, 8] as round 7 takes it"""
        d_slot = self._slots(slots)
        count = d_slot.numel()
        s_i, status = _new(self.ctx, self.L, count, 8), _new(self.ctx, count)
        N_.call.mpe_gg20_presig_sign(self.h, count, _ptr(d_slot), _ptr(msg), _ptr(s_i), _ptr(status), self.ctx.stream())
        return s_i, status

    def complete(self, slots, d_in, in_off=None):
        """`SignManual::complete` for SIGNED slots.  d_in: the partial signatures of all S senders (sender j's [count][8] block at record
        in_off[j], default j * count).  Returns dict r, s [L, count, 8], recid, status [L, count]; the slots are EMPTY afterwards."""
        d_slot = self._slots(slots)
        count, L, ctx = d_slot.numel(), self.L, self.ctx
        o = dict(r=_new(ctx, L, count, 8), s=_new(ctx, L, count, 8), recid=_new(ctx, L, count), status=_new(ctx, L, count))
        off = None if in_off is None else (C.c_int64 * self.S)(*[int(x) for x in in_off])
        N_.call.mpe_gg20_presig_complete(self.h, count, _ptr(d_slot), _ptr(d_in), off, _ptr(o["r"]), _ptr(o["s"]), _ptr(o["recid"]), _ptr(o["status"]),
                                         self.ctx.stream())
        self._pending.append((d_slot, o["status"]))          # 0 and 701 emptied the slot, 821 / 822 did not
        return o

    def sign_online(self, slots, msg):
        """The online step in one launch (mpe_gg20_sign_online; the pool holds every signer): what gg20_sign_online returns —
        r, s [count, 8], recid, status [count] (811 / 812 from the claim, 701 when the one verify fails; zero outputs unless 0)."""
        d_slot = self._slots(slots)
        count, ctx = d_slot.numel(), self.ctx
        r, s, recid, status = _new(ctx, count, 8), _new(ctx, count, 8), _new(ctx, count), _new(ctx, count)
        N_.call.mpe_gg20_sign_online(self.h, count, _ptr(d_slot), _ptr(msg), _ptr(r), _ptr(s), _ptr(recid), _ptr(status), self.ctx.stream())
        self._pending.append((d_slot, status))              # 0 and 701 emptied the slot, 811 / 812 did not
        return r, s, recid, status

    def export(self, slots, wrap=None, nonce_hi=None):
        """READY slots -> (records [count, record_words], status [count]); the slots are EMPTY afterwards, the records the only copy.
        wrap (a WrapKey): the records leave sealed, [count, sealed_words] (mpe_gg20_sealed_presig_export)"""
        d_slot = self._slots(slots)
        count = d_slot.numel()
        rec, status = _new(self.ctx, count, self.record_words if wrap is None else self.sealed_words), _new(self.ctx, count)
        if wrap is None:
            N_.call.mpe_gg20_presig_export(self.h, count, _ptr(d_slot), _ptr(rec), _ptr(status), self.ctx.stream())
        else:
            N_.call.mpe_gg20_sealed_presig_export(self.h, wrap.h, count, _ptr(d_slot), WrapKey.nonce(nonce_hi), _ptr(rec), _ptr(status), self.ctx.stream())
        self._pending.append((d_slot, status))
        return rec, status

    def import_(self, records, slots=None, wrap=None):
        """records [count, record_words] (device int32) -> free slots (or `slots`); returns the usable slots, -1 where refused.
        wrap (a WrapKey): the records are sealed rows [count, sealed_words]; a row that fails authentication is 841"""
        count = records.shape[0]
        mine = slots is None
        if mine:
            slots = self._take(count)
            self._used.update(slots)
        d_slot = self._slots(slots)
        status = _new(self.ctx, count)
        if wrap is None:
            N_.call.mpe_gg20_presig_import(self.h, count, _ptr(d_slot), _ptr(records.contiguous()), _ptr(status), self.ctx.stream())
        else:
            N_.call.mpe_gg20_sealed_presig_import(self.h, wrap.h, count, _ptr(d_slot), _ptr(records.contiguous()), _ptr(status), self.ctx.stream())
        return self._filled(d_slot.cpu().numpy(), status.cpu().numpy(), not mine)

    def discard(self, slots):
        d_slot = self._slots(slots)
        N_.call.mpe_gg20_presig_discard(self.h, d_slot.numel(), _ptr(d_slot), self.ctx.stream())
        self._pending.append((d_slot[(d_slot >= 0) & (d_slot < self.capacity)], None))

    def audit(self):
        """dict EMPTY, READY, SIGNED, BUSY (slots per state) and stray (non-zero words of k_i, sigma_i outside READY slots: must be 0)"""
        out = (C.c_int64 * 5)()
        N_.call.mpe_gg20_presig_pool_audit(self.h, out, self.ctx.stream())
        return dict(zip(self.STATES + ("stray",), [int(x) for x in out]))

    def _destroy(self):
        N_.lib.mpe_gg20_presig_pool_destroy(self.h)


def gg20_presign(ctx, keys, nonces, B, pool, keyset=None, dedup_verify=False, sigset=None):
    """The offline stage alone: rounds 0-6 of B sessions with every signer local (nonces: [B][S] layout, `msg` not needed), deposited
    into `pool` (a PresigPool over all S signers of `keys`).  Returns the usable slots [B] (numpy int32; -1 where the session failed)."""
    sess = Gg20Session(ctx, keys, B, list(range(keys.S)), nonces, keyset=keyset, dedup_verify=dedup_verify, sigset=sigset)
    try:
        prev = None
        for rnd in range(7):
            prev = sess.round(rnd, d_in=prev)                # an output [L, B, W] is the next round's input
        return pool.deposit(sess)
    finally:
        sess.close()
        ctx.wipe()                                           # the composites' workspace held nonce-derived values, as after mpe_gg20_sign


def _no_msg(ctx, nonces):
    """the nonce struct of a call that reads no message: `msg` may be missing from the dict"""
    return nonces if "msg" in nonces else dict(nonces, msg=torch.zeros((0,), dtype=torch.int32, device=ctx.device))


def gg20_presign_fused(ctx, keys, nonces, B, pool, slots=None, keyset=None, dedup_verify=False, sigset=None, chunk=0):
    """gg20_presign as ONE C call (mpe_gg20_presign_sets): rounds 0-6 chunked as gg20_sign chunks them, every chunk deposited into
    `pool` (free slots, or `slots`, one per session).  Returns the usable slots [B] (numpy int32; -1 where the row failed);
    pool.last_status holds the row statuses: the session's own status, else the deposit's 801 / 802, else 0."""
    mine = slots is None
    if mine:
        slots = pool._take(B)
        pool._used.update(slots)
    d_slot = pool._slots(slots)
    if d_slot.numel() != B:
        raise ValueError("gg20_presign_fused: one slot per session")
    d_status = torch.full((B,), -1, dtype=torch.int32, device=ctx.device)
    nn = _struct(N_.Gg20Nonces, _no_msg(ctx, nonces))
    try:
        N_.call.mpe_gg20_presign_sets(ctx.h, keys.h, B, _ptr(keyset), _ptr(sigset), C.byref(nn), pool.h, _ptr(d_slot), _ptr(d_status), int(bool(dedup_verify)),
                                      int(chunk), ctx.stream())
    except N_.MpeError:
        if mine:
            pool._used.difference_update(slots)
        raise
    return pool._filled(d_slot.cpu().numpy(), d_status.cpu().numpy(), not mine)


def gg20_sign_online(pool, slots, msg):
    """The online step for a pool that holds every signer: sign + complete.  slots: distinct READY slots; msg [count, 8].  Returns what
    gg20_sign returns: r, s [count, 8], recid, status [count] (the smallest non-zero party status, or the sign call's 811 / 812)."""
    d_slot = pool._slots(slots)
    s_i, st7 = pool.sign(d_slot, msg)
    res = pool.complete(torch.where(st7 == 0, d_slot, torch.full_like(d_slot, -1)), s_i)      # a row that lost the claim completes nothing
    st = res["status"]
    big = torch.where(st == 0, torch.full_like(st, 2 ** 31 - 1), st).amin(dim=0)
    status = torch.where(st7 != 0, st7, torch.where(big == 2 ** 31 - 1, torch.zeros_like(big), big))
    good = status == 0
    return res["r"][0] * good[:, None], res["s"][0] * good[:, None], res["recid"][0] * good, status


PLACE_PARTY, PLACE_ROTATED = 0, 1


class Comm(_Handle):
    """mpe_comm_*: the RCCL communicator of the round fan-out behind the C-ABI (include/mpecdsa_hip.h).  `exchange_id(id_or_None)`:
    a callable that carries rank 0's 128 id bytes to every rank (e.g. a torch.distributed broadcast, a file, a socket)."""
    ID_BYTES = 128

    def __init__(self, ctx, rank, world, exchange_id=None):
        self.ctx = ctx
        buf = C.create_string_buffer(self.ID_BYTES)
        if rank == 0:
            N_.call.mpe_comm_unique_id(buf)
        ident = buf.raw
        if world > 1 or exchange_id is not None:
            ident = bytes(exchange_id(ident if rank == 0 else None))
        h = C.c_void_p()
        N_.call.mpe_comm_create(ctx.h, ident, rank, world, C.byref(h))
        self.h, self.rank, self.world = h, rank, world

    def layout_self_test(self, rows_per_rank):
        mode, ok = C.c_int(-1), C.c_int(0)
        N_.call.mpe_comm_layout_self_test(self.h, rows_per_rank, C.byref(mode), C.byref(ok), self.ctx.stream())
        return dict(mode=("inplace", "copy")[mode.value], ok=bool(ok.value))

    def all_gather(self, buf, bytes_per_rank):
        N_.call.mpe_comm_all_gather(self.h, _ptr(buf), bytes_per_rank, self.ctx.stream())

    def round_exchange(self, S, n, rnd, per_rank, batch, slab):
        N_.call.mpe_gg20_round_exchange(self.h, S, n, rnd, per_rank, batch, _ptr(slab), self.ctx.stream())

    def _destroy(self):
        N_.lib.mpe_comm_destroy(self.h)


def comm_library():
    """mpe_comm_library: {"path": the librccl the communicator entry points are bound to, "adopted": it was already in the process
    (PyTorch's own copy), "version": ncclGetVersion}"""
    buf = C.create_string_buffer(4096)
    ad, ver = C.c_int(0), C.c_int(0)
    N_.call.mpe_comm_library(buf, 4096, C.byref(ad), C.byref(ver))
    return dict(path=buf.value.decode(), adopted=bool(ad.value), version=ver.value)


def shard_where(placement, S, world, block, party):
    r, s = C.c_int(0), C.c_int(0)
    N_.call.mpe_gg20_shard_where(placement, S, world, block, party, C.byref(r), C.byref(s))
    return r.value, s.value


def shard_in_off(placement, S, world, batch, block):
    off = (C.c_int64 * S)()
    N_.call.mpe_gg20_shard_in_off(placement, S, world, batch, block, off)
    return list(off)


class Gg20Pipeline(_Handle):
    """mpe_gg20_pipeline_*: a stream of `batch`-session batches, `group` of them coalesced per pass, `lanes` passes in flight on one
    stream each (include/mpecdsa_hip.h).  submit / submit_seeded return a ticket; the result tensors of a ticket are valid after
    wait(ticket) (or after stream_wait on the consuming stream).  With `pool=` (a PresigPool over all S signers of `keys`) the object is
    a PRESIG engine: submit_presig / submit_presig_seeded run the offline stage and deposit into the pool; close it before the pool."""

    def __init__(self, ctx, keys, batch, group=4, lanes=2, dedup_verify=False, pool=None):
        self.ctx, self.keys, self.batch, self.group, self.lanes, self.pool = ctx, keys, batch, group, lanes, pool
        h = C.c_void_p()
        if pool is None:
            N_.call.mpe_gg20_pipeline_create(ctx.h, keys.h, batch, group, lanes, int(bool(dedup_verify)), C.byref(h))
        else:
            N_.call.mpe_gg20_pipeline_create_presig(ctx.h, keys.h, pool.h, batch, group, lanes, int(bool(dedup_verify)), C.byref(h))
        self.h = h
        self._keep = {}                       # ticket -> the tensors the device still reads / writes

    def _outs(self, want_R):
        B = self.batch
        r, s, recid = _new(self.ctx, B, 8), _new(self.ctx, B, 8), _new(self.ctx, B)
        status = torch.full((B,), -1, dtype=torch.int32, device=self.ctx.device)
        R = _new(self.ctx, B, 16) if want_R else None
        return r, s, recid, status, R

    def submit(self, nonces, keyset=None, want_R=False, sigset=None):
        """sigset: device int32 [batch], the signer set of every session (mpe_gg20_pipeline_submit_sets)"""
        r, s, recid, status, R = self._outs(want_R)
        nn = _struct(N_.Gg20Nonces, nonces)
        t = C.c_uint64(0)
        if sigset is None:
            N_.call.mpe_gg20_pipeline_submit(self.h, _ptr(keyset), C.byref(nn), _ptr(r), _ptr(s), _ptr(recid), _ptr(R), _ptr(status), self.ctx.stream(),
                                             C.byref(t))
        else:
            N_.call.mpe_gg20_pipeline_submit_sets(self.h, _ptr(keyset), _ptr(sigset), C.byref(nn), _ptr(r), _ptr(s), _ptr(recid), _ptr(R), _ptr(status),
                                                  self.ctx.stream(), C.byref(t))
        self._keep[t.value] = ((nonces, sigset), keyset, r, s, recid, status, R)
        return t.value

    def submit_seeded(self, seed, batch_counter, msg, keyset=None, want_R=False, sigset=None):
        r, s, recid, status, R = self._outs(want_R)
        t = C.c_uint64(0)
        if sigset is None:
            N_.call.mpe_gg20_pipeline_submit_seeded(self.h, _ptr(keyset), _seed(seed), int(batch_counter), _ptr(msg), _ptr(r), _ptr(s), _ptr(recid), _ptr(R),
                                                    _ptr(status), self.ctx.stream(), C.byref(t))
        else:
            N_.call.mpe_gg20_pipeline_submit_seeded_sets(self.h, _ptr(keyset), _ptr(sigset), _seed(seed), int(batch_counter), _ptr(msg), _ptr(r), _ptr(s),
                                                         _ptr(recid), _ptr(R), _ptr(status), self.ctx.stream(), C.byref(t))
        self._keep[t.value] = ((msg, sigset), keyset, r, s, recid, status, R)
        return t.value

    # ---- the presig engine: slots come from the pool's free list (or the caller names them) and are marked used at submit; wait()
    # gives back the rows whose status is non-zero
    def _presig_slots(self, slots):
        if self.pool is None:
            raise N_.MpeError("Gg20Pipeline: submit_presig needs an engine made with pool=")
        mine = slots is None
        if mine:
            slots = self.pool._take(self.batch)
        d_slot = self.pool._slots(slots)
        if d_slot.numel() != self.batch:
            raise ValueError("submit_presig: one slot per session")
        h_slot = d_slot.cpu().numpy()
        fresh = [int(x) for x in h_slot if 0 <= x < self.pool.capacity and int(x) not in self.pool._used]     # what a failed row hands back
        self.pool._used.update(fresh)
        return d_slot, h_slot, fresh, torch.full((self.batch,), -1, dtype=torch.int32, device=self.ctx.device)

    def submit_presig(self, nonces, slots=None, keyset=None, sigset=None):
        """the offline stage of one batch into `slots` (default: free slots of the pool); wait(ticket) -> (usable slots, status)"""
        d_slot, h_slot, fresh, status = self._presig_slots(slots)
        nn = _struct(N_.Gg20Nonces, _no_msg(self.ctx, nonces))
        t = C.c_uint64(0)
        try:
            N_.call.mpe_gg20_pipeline_submit_presig(self.h, _ptr(keyset), _ptr(sigset), C.byref(nn), _ptr(d_slot), _ptr(status), self.ctx.stream(), C.byref(t))
        except N_.MpeError:
            self.pool._used.difference_update(fresh)
            raise
        self._keep[t.value] = ((nonces, sigset, d_slot), keyset, h_slot, fresh, None, status, None)
        return t.value

    def submit_presig_seeded(self, seed, batch_counter, slots=None, keyset=None, sigset=None):
        d_slot, h_slot, fresh, status = self._presig_slots(slots)
        t = C.c_uint64(0)
        try:
            N_.call.mpe_gg20_pipeline_submit_presig_seeded(self.h, _ptr(keyset), _ptr(sigset), _seed(seed), int(batch_counter), _ptr(d_slot), _ptr(status),
                                                           self.ctx.stream(), C.byref(t))
        except N_.MpeError:
            self.pool._used.difference_update(fresh)
            raise
        self._keep[t.value] = ((sigset, d_slot), keyset, h_slot, fresh, None, status, None)
        return t.value

    def flush(self):
        """sends the open group; a pass that fails is reported by its tickets (wait / ticket_rc), not here"""
        N_.lib.mpe_gg20_pipeline_flush(self.h)

    def done(self, ticket):
        """True once the batch is complete — also when its pass FAILED (ticket_rc / wait tell)"""
        d = C.c_int(0)
        N_.lib.mpe_gg20_pipeline_query(self.h, ticket, C.byref(d))
        return bool(d.value)

    def ticket_rc(self, ticket):
        """(launched, rc) of the pass that carries the batch (rc = MPE_OK while its group is still open)"""
        la, rc = C.c_int(0), C.c_int(0)
        N_.call.mpe_gg20_pipeline_ticket_rc(self.h, ticket, C.byref(la), C.byref(rc))
        return bool(la.value), rc.value

    def wait(self, ticket, want_R=False, check=True):
        """blocks until the batch is complete; returns (r, s, recid, status[, R]) and forgets the ticket's tensors.  A batch whose PASS
        failed raises MpeError (check=True) or returns its arrays — status = MPE_GG20_STATUS_PASS_FAILED(rc), no signature — with
        check=False.  A presig engine returns (usable slots [batch] numpy int32, -1 where the row's status is non-zero; status) and
        hands the slots of those rows back to the pool's free list, also when it raises."""
        rc = N_.lib.mpe_gg20_pipeline_wait(self.h, ticket)
        if ticket not in self._keep:
            N_.check(rc if rc != N_.MPE_OK else N_.MPE_E_ARG, "mpe_gg20_pipeline_wait (unknown ticket)")
        _, _, r, s, recid, status, R = self._keep.pop(ticket)
        if self.pool is not None:             # a presig ticket: r = the slots as submitted, s = those the submit marked used
            h_slot, fresh, st = r, set(s), status.cpu().numpy()
            self.pool._used.difference_update(int(x) for x in h_slot[st != 0] if int(x) in fresh)
            self.pool.last_status = st
            if check:
                N_.check(rc, "mpe_gg20_pipeline_wait")
            return np.where(st == 0, h_slot, -1).astype(np.int32), status
        if check:
            N_.check(rc, "mpe_gg20_pipeline_wait")
        return (r, s, recid, status, R) if want_R else (r, s, recid, status)

    def set_deadline_us(self, us):
        N_.call.mpe_gg20_pipeline_set_deadline_us(self.h, int(us))

    def set_eager(self, on=True):
        N_.call.mpe_gg20_pipeline_set_eager(self.h, int(bool(on)))

    def poll(self):
        la = C.c_int(0)
        N_.call.mpe_gg20_pipeline_poll(self.h, C.byref(la))
        return bool(la.value)

    def inject_fault(self, passes=1, rc=N_.MPE_E_NOMEM):
        N_.call.mpe_gg20_pipeline_inject_fault(self.h, int(passes), int(rc))

    def counters(self):
        v = [C.c_uint64(0) for _ in range(4)]
        N_.call.mpe_gg20_pipeline_counters(self.h, *[C.byref(x) for x in v])
        return dict(zip(("groups", "by_deadline", "by_idle", "failed"), (x.value for x in v)))

    def latency_ms(self, ticket):
        ms = C.c_float(0)
        N_.call.mpe_gg20_pipeline_latency_ms(self.h, ticket, C.byref(ms))
        return ms.value

    def pass_ms(self, ticket):
        ms = C.c_float(0)
        N_.call.mpe_gg20_pipeline_pass_ms(self.h, ticket, C.byref(ms))
        return ms.value

    def sampler_failures(self):
        v = C.c_int32(0)
        N_.call.mpe_gg20_pipeline_sampler_failures(self.h, C.byref(v))
        return v.value

    def _destroy(self):
        N_.lib.mpe_gg20_pipeline_destroy(self.h)
        self._keep.clear()


# ---- the sampling side of the trait surface (mpe_sample.h): curv Samplable / from_modulo / Scalar::random on the device ----
SAMPLE_NONZERO, SAMPLE_PLUS_ONE, SAMPLE_COPRIME = 1, 2, 4


def _seed(seed):
    b = bytes(seed)
    if len(b) != 32:
        raise ValueError("the sampler's seed is 32 bytes")
    return b


def sample_bits(ctx, batch, seed, stream_id, bits, out_words):
    out = _new(ctx, batch, out_words)
    N_.call.mpe_sample_bits(ctx.h, batch, _seed(seed), stream_id, bits, out_words, _ptr(out), ctx.stream())
    return out


def sample_below(ctx, batch, seed, stream_id, d_bound, out_words, d_bound_idx=None, flags=0):
    """d_bound: device int32 [nbounds, bound_words]; returns (values [batch, out_words], failures as a device int32 [1])"""
    out = _new(ctx, batch, out_words)
    fail = torch.zeros((1,), dtype=torch.int32, device=ctx.device)
    N_.call.mpe_sample_below(ctx.h, batch, _seed(seed), stream_id, _ptr(d_bound), d_bound.shape[1], d_bound.shape[0], _ptr(d_bound_idx), flags, out_words,
                             _ptr(out), _ptr(fail), ctx.stream())
    return out, fail


def sample_scalar(ctx, batch, seed, stream_id):
    out = _new(ctx, batch, 8)
    fail = torch.zeros((1,), dtype=torch.int32, device=ctx.device)
    N_.call.mpe_sample_scalar(ctx.h, batch, _seed(seed), stream_id, _ptr(out), _ptr(fail), ctx.stream())
    return out, fail


def gg20_nonce_shapes(S, n, L, B):
    """rows x words of every field of mpe_gg20_nonces (include/mpecdsa_hip.h) for B sessions x L local parties"""
    rows = wire.nonce_rows(S, n, L, B)
    return {f: (rows[f], words) for f, _, words in wire.NONCE_FIELDS}


def gg20_sample_nonces(ctx, keys, B, seed, batch_counter, local=None, keyset=None, msg=None, out=None, sigset=None, local_party=None):
    """mpe_gg20_sample_nonces: every value the local parties of B sessions draw while signing, from (seed, batch_counter).
    Returns (dict of device tensors in the layout gg20_sign / Gg20Session take, failures [1]); `msg` (device [B, 8]) is passed through."""
    by_party = local_party is not None          # (sigset / local_party: as Gg20Session takes them; mpe_gg20_sample_nonces_sets)
    local = ([int(local_party)] if by_party else list(range(keys.S))) if local is None else list(local)
    if out is None:
        out = {f: torch.zeros(shape, dtype=torch.int32, device=ctx.device) for f, shape in gg20_nonce_shapes(keys.S, keys.n, len(local), B).items()}
    if msg is not None:
        out["msg"] = msg
    fail = torch.zeros((1,), dtype=torch.int32, device=ctx.device)
    nn = _struct(N_.Gg20Nonces, out)
    lc = (C.c_int32 * len(local))(*local)
    if sigset is None and not by_party:
        N_.call.mpe_gg20_sample_nonces(ctx.h, keys.h, B, len(local), lc, _ptr(keyset), _seed(seed), int(batch_counter), C.byref(nn), _ptr(fail), ctx.stream())
    else:
        N_.call.mpe_gg20_sample_nonces_sets(ctx.h, keys.h, B, len(local), lc, _ptr(keyset), _ptr(sigset), int(by_party), _seed(seed), int(batch_counter),
                                            C.byref(nn), _ptr(fail), ctx.stream())
    return out, fail


# ---- key material (mpe_primes.h): `Keys::create` = Paillier::keypair() + generate_h1_h2_N_tilde() (party_i.rs:137-177) ----
def is_probable_prime(ctx, d_n, rounds=8):
    """d_n: device words [B, 32] -> uint8 [B]: trial division below 6370, then `rounds` Miller-Rabin tests to the FIXED bases 2, 3, 5, ..."""
    ok = _flags(ctx, d_n.shape[0])
    N_.call.mpe_is_probable_prime(ctx.h, d_n.shape[0], _ptr(d_n), rounds, _ptr(ok), ctx.stream())
    return ok


def sample_prime(ctx, batch, seed, stream_id, bits=1024, max_attempts=0):
    """kzen-paillier sample_prime per item: (primes [batch, 32], attempt [batch] (-1: gave up), failures [1])"""
    out = _new(ctx, batch, bits // 32)
    attempt = torch.zeros((batch,), dtype=torch.int32, device=ctx.device)
    fail = torch.zeros((1,), dtype=torch.int32, device=ctx.device)
    N_.call.mpe_sample_prime(ctx.h, batch, _seed(seed), stream_id, bits, max_attempts, _ptr(out), _ptr(attempt), _ptr(fail), ctx.stream())
    return out, attempt, fail


def sample_safe_prime(ctx, batch, seed, stream_id, bits=1024, max_attempts=0):
    """kzen-paillier sample_safe_prime per item — the lowest attempt of sample_prime's sequence whose candidate c and (c - 1) / 2 are both
    prime: (primes [batch, 32], attempt [batch] (-1: gave up), failures [1]); max_attempts 0 = 2^24"""
    out = _new(ctx, batch, bits // 32)
    attempt = torch.zeros((batch,), dtype=torch.int32, device=ctx.device)
    fail = torch.zeros((1,), dtype=torch.int32, device=ctx.device)
    N_.call.mpe_sample_safe_prime(ctx.h, batch, _seed(seed), stream_id, bits, max_attempts, _ptr(out), _ptr(attempt), _ptr(fail), ctx.stream())
    return out, attempt, fail


def prime_search_counts(ctx, reset=False):
    """what this context's prime searches counted so far, a measurement aid: attempts sieved and the length of the list behind each stage,
    for the plain search (3 figures) and the safe one (6)"""
    v = (C.c_int64 * 9)()
    N_.call.mpe_prime_search_counts(ctx.h, v, int(reset))
    names = ("attempts", "sieve", "round1", "safe_attempts", "safe_sieve_head", "safe_sieve", "safe_round1_c", "safe_round1_half", "safe_rounds2_8_c")
    return dict(zip(names, (int(x) for x in v)))


def paillier_keygen(ctx, nkeys, seed, counter, max_attempts=0, safe_primes=False):
    """`Paillier::keypair()` x nkeys — `Paillier::keypair_safe_primes()` with safe_primes=True (one (seed, counter) mints one key: the plain or
    the safe one): device (p [nkeys, 32], q [nkeys, 32], N [nkeys, 64], failures [1]); PaillierKeys(ctx, p=p, q=q) takes p, q"""
    p, q, n = _new(ctx, nkeys, 32), _new(ctx, nkeys, 32), _new(ctx, nkeys, 64)
    fail = torch.zeros((1,), dtype=torch.int32, device=ctx.device)
    name = "mpe_paillier_keygen_safe_primes" if safe_primes else "mpe_paillier_keygen"
    getattr(N_.call, name)(ctx.h, nkeys, _seed(seed), int(counter), max_attempts, _ptr(p), _ptr(q), _ptr(n), _ptr(fail), ctx.stream())
    return p, q, n, fail


def ntilde_generate(ctx, count, seed, counter, max_attempts=0, safe_primes=False):
    """`generate_h1_h2_N_tilde()` x count (safe_primes=True: p~, q~ are safe primes, as the reference's comment asks): dict of device [count, 64]
    tensors Nt, h1, h2 (Statements(ctx, Nt, h1, h2) takes them), xhi, xhi_inv and the failures [1]"""
    o = {f: _new(ctx, count, 64) for f in ("Nt", "h1", "h2", "xhi", "xhi_inv")}
    fail = torch.zeros((1,), dtype=torch.int32, device=ctx.device)
    name = "mpe_ntilde_generate_safe_primes" if safe_primes else "mpe_ntilde_generate"
    getattr(N_.call, name)(ctx.h, count, _seed(seed), int(counter), max_attempts, _ptr(o["Nt"]), _ptr(o["h1"]), _ptr(o["h2"]), _ptr(o["xhi"]),
                           _ptr(o["xhi_inv"]), _ptr(fail), ctx.stream())
    o["fail"] = fail
    return o


# ---- keygen verification math (gg_2020/party_i.rs:260-438) ----
def correct_key_verify(ctx, d_N, d_sigma):
    ok = _flags(ctx, d_N.shape[0])
    N_.call.mpe_correct_key_verify(ctx.h, d_N.shape[0], _ptr(d_N), _ptr(d_sigma), _ptr(ok), ctx.stream())
    return ok


def composite_dlog_verify(ctx, d_N, d_g, d_ni, d_x, d_y):
    ok = _flags(ctx, d_N.shape[0])
    N_.call.mpe_composite_dlog_verify(ctx.h, d_N.shape[0], _ptr(d_N), _ptr(d_g), _ptr(d_ni), _ptr(d_x), _ptr(d_y), _ptr(ok), ctx.stream())
    return ok


def keygen_verify_round1(ctx, n_parties, msgs):
    """`phase1_verify_com_phase3_verify_correct_key_verify_dlog_phase2_distribute` (party_i.rs:260-320) over items = (session, prover):
    msgs = dict of device tensors (fields _native.KEYGEN_ROUND1_FIELDS).  Returns (ok [B] uint8, bad_actors [B / n_parties] int32 masks)."""
    B = msgs["N"].shape[0]
    ok = _flags(ctx, B)
    bad = torch.zeros((B // n_parties,), dtype=torch.int32, device=ctx.device)
    st = _struct(N_.KeygenRound1, msgs)
    N_.call.mpe_keygen_verify_round1(ctx.h, B, n_parties, C.byref(st), _ptr(ok), _ptr(bad), ctx.stream())
    return ok, bad


def keygen_verify_round2(ctx, n_parties, t1, d_commits, d_share, d_index, d_y):
    """the verdict of `phase2_verify_vss_construct_keypair_phase3_pok_dlog` (party_i.rs:322-367)"""
    B = d_share.shape[0]
    ok = _flags(ctx, B)
    bad = torch.zeros((B // n_parties,), dtype=torch.int32, device=ctx.device)
    N_.call.mpe_keygen_verify_round2(ctx.h, B, n_parties, t1, _ptr(d_commits), _ptr(d_share), _ptr(d_index), _ptr(d_y), _ptr(ok), _ptr(bad), ctx.stream())
    return ok, bad


def correct_key_prove(ctx, sk):
    """`NiCorrectKeyProof::proof` for every key of a private key set: sigma [nkeys, 11, 64]"""
    sigma = torch.zeros((sk.nkeys, 11, 64), dtype=torch.int32, device=ctx.device)
    N_.call.mpe_correct_key_prove(ctx.h, sk.h, _ptr(sigma), ctx.stream())
    return sigma


def composite_dlog_prove(ctx, d_N, d_g, d_ni, d_secret, d_r):
    B = d_N.shape[0]
    x, y = _new(ctx, B, 64), _new(ctx, B, 73)
    N_.call.mpe_composite_dlog_prove(ctx.h, B, _ptr(d_N), _ptr(d_g), _ptr(d_ni), _ptr(d_secret), _ptr(d_r), _ptr(x), _ptr(y), ctx.stream())
    return x, y


def vss_validate_share(ctx, t1, d_commits, d_share, d_index):
    ok = _flags(ctx, d_share.shape[0])
    N_.call.mpe_vss_validate_share(ctx.h, d_share.shape[0], t1, _ptr(d_commits), _ptr(d_share), _ptr(d_index), _ptr(ok), ctx.stream())
    return ok


def vss_point_commitment(ctx, t1, d_commits, d_index):
    out = _new(ctx, d_index.shape[0], 16)
    N_.call.mpe_vss_point_commitment(ctx.h, d_index.shape[0], t1, _ptr(d_commits), _ptr(d_index), _ptr(out), ctx.stream())
    return out


# ---- the rest of keygen: dealing, the key pair, round 3 (gg_2020/party_i.rs:260-438) ----
def vss_share(ctx, n, d_coef):
    """`VerifiableSS::share(t, n, &u_i)` per dealer: d_coef [B, t+1, 8] (coef[0] = u_i) -> (commits [B, t+1, 16], shares [B, n, 8]),
    shares[b, j] = f_b(j + 1).  A zero coefficient gives a neutral commitment row, which vss_validate_share refuses."""
    B, t1 = d_coef.shape[0], d_coef.shape[1]
    commits, shares = _new(ctx, B, t1, 16), _new(ctx, B, n, 8)
    N_.call.mpe_vss_share(ctx.h, B, t1, n, _ptr(d_coef), _ptr(commits), _ptr(shares), ctx.stream())
    return commits, shares


def keygen_construct_keypair(ctx, d_shares, d_y, d_nonce):
    """the OK branch of `phase2_verify_vss_construct_keypair_phase3_pok_dlog` (party_i.rs:355-363) over items = (session, receiving party):
    d_shares [B, n, 8] received shares in dealer order, d_y [B, n, 16], d_nonce [B, 8] -> (x, ysum, pk, R, z); (pk, R, z) = dlog_prove(x, nonce)"""
    B, n = d_shares.shape[0], d_shares.shape[1]
    x, ysum, pk, R, z = _new(ctx, B, 8), _new(ctx, B, 16), _new(ctx, B, 16), _new(ctx, B, 16), _new(ctx, B, 8)
    N_.call.mpe_keygen_construct_keypair(ctx.h, B, n, _ptr(d_shares), _ptr(d_y), _ptr(d_nonce), _ptr(x), _ptr(ysum), _ptr(pk), _ptr(R), _ptr(z), ctx.stream())
    return x, ysum, pk, R, z


def keygen_verify_round3(ctx, n_parties, d_commits, d_pk, d_R, d_z, want_xi=False):
    """`Keys::verify_dlog_proofs_check_against_vss` (party_i.rs:405-438) over items (session, i) = dealer i's commitments
    d_commits [B, t+1, 16] and party i's proof.  Returns (ok [B] uint8, bad_actors [B / n_parties] int32 masks[, xi_commit [B, 16]])."""
    B, t1 = d_commits.shape[0], d_commits.shape[1]
    ok = _flags(ctx, B)
    bad = torch.zeros((B // n_parties,), dtype=torch.int32, device=ctx.device)
    xi = _new(ctx, B, 16) if want_xi else None
    N_.call.mpe_keygen_verify_round3(ctx.h, B, n_parties, t1, _ptr(d_commits), _ptr(d_pk), _ptr(d_R), _ptr(d_z), _ptr(ok), _ptr(bad), _ptr(xi), ctx.stream())
    return (ok, bad, xi) if want_xi else (ok, bad)


KEYGEN_MATERIAL_FIELDS = ("p", "q", "pt", "qt", "h1", "xi")        # rows [B*n, 32] x 4, [B*n, 64] x 2


def gg20_keygen(ctx, t, n, B, seed, counter=0, material=None, _fault=None, safe_primes=False, safe_ntilde=False, wrap=None, nonce_hi=None):
    """`Keygen` (gg_2020/state_machine/keygen/rounds.rs) for B wallets in lock step with all n parties local, the counterpart of gg20_sign:
    a chain of C-ABI calls, rows = (wallet, party).
      material: None = mint the Paillier / N~ material on the device (streams counter | 0..5 << 56 of `seed`); or a dict of uint32
                arrays KEYGEN_MATERIAL_FIELDS (p, q, p~, q~ [B n, 32]; h1, xi [B n, 64]) taken as generate_h1_h2_N_tilde would have
                drawn them (N, N~, h2 = h1^xi and the two proof secrets are derived on the host).
      safe_primes: mint every party's Paillier key from safe primes — `Keys::create_safe_prime` (party_i.rs:179-199), the key generation
                the reference recommends for production; safe_ntilde additionally mints N~ from safe primes (its "note, should be safe
                primes").  Both only apply to material minted here; a safe prime costs ~1000 plain ones.
      u_i, blind factors, VSS coefficients, the DLog nonces and the two CompositeDLog nonces: streams counter | 8..13 << 56.
      _fault:   a test aid, not part of the interface: (wallet, dealer, party) flips bit 0 of the share that dealer sends to that party
                before round 2, as Gg20Session.fault_inject does for signing (tests/test_keygen_deal_gpu.py walks the blame path with it).
    Returns a dict: ok [B] uint8 (all three verdicts of every party), bad1 [B] (provers of round 1), bad2 [B, n] (per receiving party,
    the dealers round 2 blames), bad3 [B] (round 3), commits [B n, t+1, 16], xi_commit [B n, 16], failures (sampler / prime search
    give-ups) and `arrays`, the layout Gg20Keys takes with nkeysets = B.
      wrap:     a WrapKey: every party's x_i, p, q are sealed on the device (mpe_gg20_keyshare_seal) before anything is copied out;
                `arrays` then has no x, p, q and the dict carries `sealed_shares` [B n, 82] (numpy uint32) for Gg20Keys(sealed_shares=)."""
    P, t1 = B * n, t + 1
    if counter >> 56:
        raise ValueError("counter < 2^56")
    sid = lambda f: int(counter) | (f << 56)
    fails = []
    if material is not None and (safe_primes or safe_ntilde):
        raise ValueError("safe_primes / safe_ntilde apply to material minted on the device")
    if material is None:
        p, q, N, f = paillier_keygen(ctx, P, seed, counter, safe_primes=safe_primes)
        nt = ntilde_generate(ctx, P, seed, counter, safe_primes=safe_ntilde)
        Nt, h1, h2, xhi, xhi_inv = nt["Nt"], nt["h1"], nt["h2"], nt["xhi"], nt["xhi_inv"]
        fails += [f, nt["fail"]]
    else:
        m = {f: words_to_ints(np.ascontiguousarray(material[f])) for f in KEYGEN_MATERIAL_FIELDS}
        if any(len(v) != P for v in m.values()):
            raise ValueError("material: B * n rows per field")
        phi = [(a - 1) * (b - 1) for a, b in zip(m["pt"], m["qt"])]
        nts = [a * b for a, b in zip(m["pt"], m["qt"])]
        up = lambda vals, w: dev(ctx, vals, w)
        p, q, N = up(m["p"], 32), up(m["q"], 32), up([a * b for a, b in zip(m["p"], m["q"])], 64)
        Nt, h1 = up(nts, 64), up(m["h1"], 64)
        h2 = up([pow(h, x, nn) for h, x, nn in zip(m["h1"], m["xi"], nts)], 64)
        xhi = up([f_ - x for f_, x in zip(phi, m["xi"])], 64)
        xhi_inv = up([f_ - pow(x, -1, f_) for f_, x in zip(phi, m["xi"])], 64)
    u, f = sample_scalar(ctx, P, seed, sid(8))
    fails.append(f)
    blind = sample_bits(ctx, P, seed, sid(9), 256, 8)
    coef = u.reshape(P, 1, 8)
    if t:
        a, f = sample_scalar(ctx, P * t, seed, sid(10))
        fails.append(f)
        coef = torch.cat([coef, a.reshape(P, t, 8)], dim=1).contiguous()
    nonce, f = sample_scalar(ctx, P, seed, sid(11))
    fails.append(f)
    r1, r2 = sample_bits(ctx, P, seed, sid(12), 512, 16), sample_bits(ctx, P, seed, sid(13), 512, 16)
    # round 1 (party_i.rs:219-320): y_i = u_i G, its hash commitment, NiCorrectKeyProof, the two CompositeDLogProofs; every prover is verified
    y = ec_mul_base(ctx, u)
    sk = PaillierKeys(ctx, p=p, q=q)
    msgs = dict(y=y, blind=blind, com=hash_commit_point(ctx, y, blind), N=N, sigma=correct_key_prove(ctx, sk).reshape(P, 11 * 64), Nt=Nt, h1=h1, h2=h2)
    msgs["x_h1"], msgs["y_h1"] = composite_dlog_prove(ctx, Nt, h1, h2, xhi, r1)
    msgs["x_h2"], msgs["y_h2"] = composite_dlog_prove(ctx, Nt, h2, h1, xhi_inv, r2)
    ok1, bad1 = keygen_verify_round1(ctx, n, msgs)
    sk.close()
    # round 2 (:322-367): deal, then party r checks dealer j's share: items ((wallet, r), j)
    commits, shares = vss_share(ctx, n, coef)
    recv = shares.reshape(B, n, n, 8).transpose(1, 2).contiguous()                     # [wallet, receiver, dealer]
    if _fault is not None:
        w_, j_, r_ = _fault
        recv[w_, r_, j_, 0] ^= 1
    c_it = commits.reshape(B, 1, n, t1 * 16).expand(B, n, n, t1 * 16).reshape(P * n, t1 * 16).contiguous()
    y_it = y.reshape(B, 1, n, 16).expand(B, n, n, 16).contiguous()
    idx = (torch.arange(n, dtype=torch.int32, device=ctx.device) + 1).reshape(1, n, 1).expand(B, n, n).reshape(P * n).contiguous()
    ok2, bad2 = keygen_verify_round2(ctx, n, t1, c_it, recv.reshape(P * n, 8), idx, y_it.reshape(P * n, 16))
    # :355-363 and round 3 (:405-438)
    x, ysum, pk, R, z = keygen_construct_keypair(ctx, recv.reshape(P, n, 8), y_it.reshape(P, n, 16), nonce)
    ok3, bad3, xi = keygen_verify_round3(ctx, n, commits, pk, R, z, want_xi=True)
    ok = ok1.reshape(B, n).bool().all(1) & ok2.reshape(B, n * n).bool().all(1) & ok3.reshape(B, n).bool().all(1)
    ctx.sync()
    secret = dict(x=x, p=p, q=q)
    sealed_shares = None
    if wrap is not None:
        sealed_shares = _to_np_u32(keyshare_seal(ctx, wrap, x, p, q, nonce_hi))
        secret = {}
    arrays = {f: _to_np_u32(v) for f, v in dict(secret, N=N, Nt=Nt, h1=h1, h2=h2, X=pk).items()}
    arrays["y"] = np.ascontiguousarray(_to_np_u32(ysum).reshape(B, n, 16)[:, 0])
    out = dict(ok=ok.to(torch.uint8), bad1=bad1, bad2=bad2.reshape(B, n), bad3=bad3, commits=commits, xi_commit=xi,
               failures=int(sum(int(f.item()) for f in fails)), arrays=arrays)
    if wrap is not None:
        out["sealed_shares"] = sealed_shares
    return out


# ---- identifiable abort (gg_2020/blame.rs) ----
def gg20_blame5(ctx, keys, B, opened, keyset=None, sigset=None):
    """opened: dict of device tensors (fields _native.Blame5In) -> bad_actors bit masks [B] (device int32); sigset: the sessions' signer
    sets (mpe_gg20_blame5_sets)"""
    bad = _new(ctx, B)
    st_ = _struct(N_.Blame5In, opened)
    if sigset is None:
        N_.call.mpe_gg20_blame5(ctx.h, keys.h, B, _ptr(keyset), C.byref(st_), _ptr(bad), ctx.stream())
    else:
        N_.call.mpe_gg20_blame5_sets(ctx.h, keys.h, B, _ptr(keyset), _ptr(sigset), C.byref(st_), _ptr(bad), ctx.stream())
    return bad


def gg20_blame6(ctx, keys, B, opened, keyset=None, sigset=None):
    bad = _new(ctx, B)
    st_ = _struct(N_.Blame6In, opened)
    if sigset is None:
        N_.call.mpe_gg20_blame6(ctx.h, keys.h, B, _ptr(keyset), C.byref(st_), _ptr(bad), ctx.stream())
    else:
        N_.call.mpe_gg20_blame6_sets(ctx.h, keys.h, B, _ptr(keyset), _ptr(sigset), C.byref(st_), _ptr(bad), ctx.stream())
    return bad


def gg20_blame7(ctx, S, B, opened):
    bad = _new(ctx, B)
    st_ = _struct(N_.Blame7In, opened)
    N_.call.mpe_gg20_blame7(ctx.h, S, B, C.byref(st_), _ptr(bad), ctx.stream())
    return bad


def ecddh_prove(ctx, d_x, d_s, statement):
    B = d_x.shape[0]
    out = dict(a1=_new(ctx, B, 16), a2=_new(ctx, B, 16), z=_new(ctx, B, 8))
    stt, pr = _struct(N_.EcddhStatement, statement), _struct(N_.EcddhProof, out)
    N_.call.mpe_ecddh_prove(ctx.h, B, _ptr(d_x), _ptr(d_s), C.byref(stt), C.byref(pr), ctx.stream())
    return out


def ecddh_verify(ctx, statement, proof):
    B = proof["z"].shape[0]
    ok = _flags(ctx, B)
    stt, pr = _struct(N_.EcddhStatement, statement), _struct(N_.EcddhProof, proof)
    N_.call.mpe_ecddh_verify(ctx.h, B, C.byref(stt), C.byref(pr), _ptr(ok), ctx.stream())
    return ok


# ---- curv sigma proofs of phases 3 / 6, the phase-1 commitment (device-tensor API) ----
def pedersen_prove(ctx, d_m, d_r, d_s1, d_s2):
    B = d_m.shape[0]
    out = dict(com=_new(ctx, B, 16), e=_new(ctx, B, 8), a1=_new(ctx, B, 16), a2=_new(ctx, B, 16), z1=_new(ctx, B, 8), z2=_new(ctx, B, 8))
    pr = _struct(N_.PedersenProof, out)
    N_.call.mpe_pedersen_prove(ctx.h, B, _ptr(d_m), _ptr(d_r), _ptr(d_s1), _ptr(d_s2), C.byref(pr), ctx.stream())
    return out


def pedersen_verify(ctx, proof):
    B = proof["com"].shape[0]
    ok = _flags(ctx, B)
    pr = _struct(N_.PedersenProof, proof)
    N_.call.mpe_pedersen_verify(ctx.h, B, C.byref(pr), _ptr(ok), ctx.stream())
    return ok


def heg_prove(ctx, d_x, d_r, d_s1, d_s2, statement):
    B = d_x.shape[0]
    out = dict(T=_new(ctx, B, 16), A3=_new(ctx, B, 16), z1=_new(ctx, B, 8), z2=_new(ctx, B, 8))
    stt, pr = _struct(N_.HegStatement, statement), _struct(N_.HegProof, out)
    N_.call.mpe_heg_prove(ctx.h, B, _ptr(d_x), _ptr(d_r), _ptr(d_s1), _ptr(d_s2), C.byref(stt), C.byref(pr), ctx.stream())
    return out


def heg_verify(ctx, statement, proof):
    B = proof["T"].shape[0]
    ok = _flags(ctx, B)
    stt, pr = _struct(N_.HegStatement, statement), _struct(N_.HegProof, proof)
    N_.call.mpe_heg_verify(ctx.h, B, C.byref(stt), C.byref(pr), _ptr(ok), ctx.stream())
    return ok


def hash_commit_point(ctx, d_P, d_blind):
    out = _new(ctx, d_P.shape[0], 8)
    N_.call.mpe_hash_commit_point(ctx.h, d_P.shape[0], _ptr(d_P), _ptr(d_blind), _ptr(out), ctx.stream())
    return out


BOB_PROOF_WORDS = dict(t=64, z=64, e=8, s=64, s1=25, s2=89, t1=81, t2=89)
BOB_NONCE_WORDS = dict(alpha=24, beta=64, gamma=80, rho=72, rho_prim=88, sigma=72, tau=88)


def bob_generate(ctx, pk, stm, d_a_enc, d_mta_enc, d_b, d_beta_prim, d_r, nonces, check, d_key_idx=None, d_st_idx=None):
    """`BobProof::generate(a_encrypted, mta_encrypted, b, beta_prim, alice_ek, dlog_statement, r, check)` batched.
    Returns (proof dict, u or None)."""
    B = d_b.shape[0]
    out = {f: _new(ctx, B, w) for f, w in BOB_PROOF_WORDS.items()}
    u = _new(ctx, B, 16) if check else None
    nn, pr = _struct(N_.BobNonces, nonces), _struct(N_.BobProof, out)
    N_.call.mpe_bob_generate(ctx.h, pk.h, stm.h, B, _ptr(d_key_idx), _ptr(d_st_idx), _ptr(d_a_enc), _ptr(d_mta_enc), _ptr(d_b), _ptr(d_beta_prim), _ptr(d_r),
                             C.byref(nn), int(bool(check)), C.byref(pr), _ptr(u), ctx.stream())
    return out, u


def bob_verify(ctx, pk, stm, d_a_enc, d_mta_enc, proof, d_X=None, d_u=None, d_key_idx=None, d_st_idx=None):
    """`BobProof::verify` (d_X, d_u None) / `BobProofExt::verify` batched -> ok flags"""
    B = d_a_enc.shape[0]
    ok = _flags(ctx, B)
    pr = _struct(N_.BobProof, proof)
    N_.call.mpe_bob_verify(ctx.h, pk.h, stm.h, B, _ptr(d_key_idx), _ptr(d_st_idx), _ptr(d_a_enc), _ptr(d_mta_enc), C.byref(pr), _ptr(d_X), _ptr(d_u), _ptr(ok),
                           ctx.stream())
    return ok


# ================================================================================================
# MtA (src/utilities/mta/mod.rs): MessageA / MessageB / verify_proofs_get_alpha, batched
# ================================================================================================
def mta_message_a(ctx, pk, stm, d_a, d_r, nonces, d_key_idx=None):
    """`MessageA::a_with_predefined_randomness`: returns (c [B,128], range proofs dict [B*nst, ...])"""
    B, total = d_a.shape[0], d_a.shape[0] * stm.count
    c = _new(ctx, B, 128)
    proofs = {f: _new(ctx, total, w) for f, w in ALICE_PROOF_WORDS.items()}
    nn, pr = _struct(N_.AliceNonces, nonces), _struct(N_.AliceProof, proofs)
    N_.call.mpe_mta_message_a(ctx.h, pk.h, stm.h, B, _ptr(d_key_idx), _ptr(d_a), _ptr(d_r), C.byref(nn), _ptr(c), C.byref(pr), ctx.stream())
    return c, proofs


def mta_message_b(ctx, pk, stm, d_b, d_ca, range_proofs, d_r, d_beta_tag, d_nonce_b, d_nonce_bt, d_key_idx=None):
    """`MessageB::b_with_predefined_randomness`: returns dict(c, beta, b_proof, beta_tag_proof, ok)"""
    B = d_b.shape[0]
    out = dict(c=_new(ctx, B, 128), beta=_new(ctx, B, 8), ok=_flags(ctx, B),
               b_proof=dict(pk=_new(ctx, B, 16), R=_new(ctx, B, 16), z=_new(ctx, B, 8)),
               beta_tag_proof=dict(pk=_new(ctx, B, 16), R=_new(ctx, B, 16), z=_new(ctx, B, 8)))
    rp = _struct(N_.AliceProof, range_proofs)
    p1, p2 = _struct(N_.DlogProof, out["b_proof"]), _struct(N_.DlogProof, out["beta_tag_proof"])
    N_.call.mpe_mta_message_b(ctx.h, pk.h, stm.h, B, _ptr(d_key_idx), _ptr(d_b), _ptr(d_ca), C.byref(rp), _ptr(d_r), _ptr(d_beta_tag), _ptr(d_nonce_b),
                              _ptr(d_nonce_bt), _ptr(out["c"]), _ptr(out["beta"]), C.byref(p1), C.byref(p2), _ptr(out["ok"]), ctx.stream())
    return out


def mta_verify_get_alpha(ctx, sk, d_cb, b_proof, beta_tag_proof, d_a, d_key_idx=None):
    """`MessageB::verify_proofs_get_alpha(dk, a)`: returns (alpha [B,8], alice_share [B,64], ok)"""
    B = d_cb.shape[0]
    alpha, share, ok = _new(ctx, B, 8), _new(ctx, B, 64), _flags(ctx, B)
    p1, p2 = _struct(N_.DlogProof, b_proof), _struct(N_.DlogProof, beta_tag_proof)
    N_.call.mpe_mta_verify_get_alpha(ctx.h, sk.h, B, _ptr(d_key_idx), _ptr(d_cb), C.byref(p1), C.byref(p2), _ptr(d_a), _ptr(alpha), _ptr(share), _ptr(ok),
                                     ctx.stream())
    return alpha, share, ok


# ---- Lindell'17 two-party ECDSA, signing (lindell_2017/party_two.rs:390-423, party_one.rs:519-565) ----
def lindell_partial_sig(ctx, pk, d_c_key, d_x2, d_k2, d_R1, d_msg, d_rho, d_r, d_key_idx=None):
    """`PartialSig::compute` batched: returns c3 [B,128] (device)."""
    B = d_c_key.shape[0]
    c3 = _new(ctx, B, 128)
    N_.call.mpe_lindell_partial_sig(ctx.h, pk.h, B, _ptr(d_key_idx), _ptr(d_c_key), _ptr(d_x2), _ptr(d_k2), _ptr(d_R1), _ptr(d_msg), _ptr(d_rho), _ptr(d_r),
                                    _ptr(c3), ctx.stream())
    return c3


def paillier_open(ctx, sk, d_c, d_key_idx=None):
    """kzen-paillier `Open::open`: returns (m [B,64], r [B,64]) with c = (1 + m N) r^N mod N^2."""
    B = d_c.shape[0]
    m, r = _new(ctx, B, 64), _new(ctx, B, 64)
    N_.call.mpe_paillier_open(ctx.h, sk.h, B, _ptr(d_key_idx), _ptr(d_c), _ptr(m), _ptr(r), ctx.stream())
    return m, r


def lindell_pdl_proof(ctx, sk, stm, d_c_key, d_x1, d_r, nonces, d_key_idx=None, d_st_idx=None):
    """party one's `pdl_proof` (party_one.rs:366-401): returns (Q [B,16], proof dict)."""
    B = d_x1.shape[0]
    out = {f: _new(ctx, B, w) for f, w in PDL_PROOF_WORDS.items()}
    Q = _new(ctx, B, 16)
    nn, pr = _struct(N_.PdlNonces, nonces), _struct(N_.PdlProof, out)
    N_.call.mpe_lindell_pdl_proof(ctx.h, sk.h, stm.h, B, _ptr(d_key_idx), _ptr(d_st_idx), _ptr(d_c_key), _ptr(d_x1), _ptr(d_r), C.byref(nn), _ptr(Q),
                                  C.byref(pr), ctx.stream())
    return Q, out


def lindell_pdl_verify(ctx, pk, d_Nt, d_h1, d_h2, d_dlog_x, d_dlog_y, d_stmt_N, d_stmt_c, d_stmt_Q, d_c_key, d_q1, proof, d_key_idx=None):
    """party two's `PaillierPublic::pdl_verify` (party_two.rs:275-300): ok flags [B]."""
    B = d_stmt_c.shape[0]
    ok = _flags(ctx, B)
    pr = _struct(N_.PdlProof, proof)
    N_.call.mpe_lindell_pdl_verify(ctx.h, pk.h, B, _ptr(d_key_idx), _ptr(d_Nt), _ptr(d_h1), _ptr(d_h2), _ptr(d_dlog_x), _ptr(d_dlog_y), _ptr(d_stmt_N),
                                   _ptr(d_stmt_c), _ptr(d_stmt_Q), _ptr(d_c_key), _ptr(d_q1), C.byref(pr), _ptr(ok), ctx.stream())
    return ok


def lindell_sign(ctx, sk, d_c3, d_k1, d_R2, d_key_idx=None):
    """`Signature::compute_with_recid` batched: returns (r [B,8], s [B,8], recid [B]) on the device."""
    B = d_c3.shape[0]
    r, s, recid = _new(ctx, B, 8), _new(ctx, B, 8), _new(ctx, B)
    N_.call.mpe_lindell_sign(ctx.h, sk.h, B, _ptr(d_key_idx), _ptr(d_c3), _ptr(d_k1), _ptr(d_R2), _ptr(r), _ptr(s), _ptr(recid), ctx.stream())
    return r, s, recid


# ---- Lindell'17, key generation and the ephemeral exchange (mpe_lindell_keygen.h; lindell_2017/party_one.rs, party_two.rs) ----
def hash_commit_bigint(ctx, d_m, d_blind):
    """HashCommitment over a 256-bit BigInt m [B,8] (minimal bytes, as the blind factor): com [B,8]"""
    out = _new(ctx, d_m.shape[0], 8)
    N_.call.mpe_hash_commit_bigint(ctx.h, d_m.shape[0], _ptr(d_m), _ptr(d_blind), _ptr(out), ctx.stream())
    return out


def lindell_keygen_first_msg(ctx, d_x1, d_nonce, d_blind_pk, d_blind_pok):
    """party one's `KeyGenFirstMsg::create_commitments_with_fixed_secret_share` (party_one.rs:179-219): dict Q1, R, z, pk_com, pok_com"""
    B = d_x1.shape[0]
    o = dict(Q1=_new(ctx, B, 16), R=_new(ctx, B, 16), z=_new(ctx, B, 8), pk_com=_new(ctx, B, 8), pok_com=_new(ctx, B, 8))
    N_.call.mpe_lindell_keygen_first_msg(ctx.h, B, _ptr(d_x1), _ptr(d_nonce), _ptr(d_blind_pk), _ptr(d_blind_pok), _ptr(o["Q1"]), _ptr(o["R"]), _ptr(o["z"]),
                                         _ptr(o["pk_com"]), _ptr(o["pok_com"]), ctx.stream())
    return o


def lindell_keygen_verify_first_msg(ctx, d_pk_com, d_pok_com, d_blind_pk, d_blind_pok, d_Q1, d_R, d_z):
    """party two's `KeyGenSecondMsg::verify_commitments_and_dlog_proof` (party_two.rs:180-223): ok [B]"""
    ok = _flags(ctx, d_Q1.shape[0])
    N_.call.mpe_lindell_keygen_verify_first_msg(ctx.h, d_Q1.shape[0], _ptr(d_pk_com), _ptr(d_pok_com), _ptr(d_blind_pk), _ptr(d_blind_pok), _ptr(d_Q1),
                                                _ptr(d_R), _ptr(d_z), _ptr(ok), ctx.stream())
    return ok


def lindell_eph_first_msg(ctx, d_k2, d_nonce, d_blind_pk, d_blind_pok):
    """party two's `EphKeyGenFirstMsg::create_commitments` (party_two.rs:315-371): dict pub, c, a1, a2, z, pk_com, pok_com"""
    B = d_k2.shape[0]
    o = dict(pub=_new(ctx, B, 16), c=_new(ctx, B, 16), a1=_new(ctx, B, 16), a2=_new(ctx, B, 16), z=_new(ctx, B, 8), pk_com=_new(ctx, B, 8),
             pok_com=_new(ctx, B, 8))
    N_.call.mpe_lindell_eph_first_msg(ctx.h, B, _ptr(d_k2), _ptr(d_nonce), _ptr(d_blind_pk), _ptr(d_blind_pok), _ptr(o["pub"]), _ptr(o["c"]), _ptr(o["a1"]),
                                      _ptr(o["a2"]), _ptr(o["z"]), _ptr(o["pk_com"]), _ptr(o["pok_com"]), ctx.stream())
    return o


def lindell_eph_verify_first_msg(ctx, d_pk_com, d_pok_com, d_blind_pk, d_blind_pok, d_pub, d_c, d_a1, d_a2, d_z):
    """party one's `EphKeyGenSecondMsg::verify_commitments_and_dlog_proof` (party_one.rs:437-483): ok [B]"""
    ok = _flags(ctx, d_pub.shape[0])
    N_.call.mpe_lindell_eph_verify_first_msg(ctx.h, d_pub.shape[0], _ptr(d_pk_com), _ptr(d_pok_com), _ptr(d_blind_pk), _ptr(d_blind_pok), _ptr(d_pub),
                                             _ptr(d_c), _ptr(d_a1), _ptr(d_a2), _ptr(d_z), _ptr(ok), ctx.stream())
    return ok


def ecdsa_verify(ctx, d_pub, d_msg, d_r, d_s):
    """`party_one::verify` (party_one.rs:567-592) batched: ok [B]; high s and s >= q are refused, r is compared with P.x as integers"""
    ok = _flags(ctx, d_pub.shape[0])
    N_.call.mpe_ecdsa_verify(ctx.h, d_pub.shape[0], _ptr(d_pub), _ptr(d_msg), _ptr(d_r), _ptr(d_s), _ptr(ok), ctx.stream())
    return ok


def scalar_mul(ctx, d_a, d_b):
    """a b mod q per row [B,8]"""
    out = _new(ctx, d_a.shape[0], 8)
    N_.call.mpe_scalar_mul(ctx.h, d_a.shape[0], _ptr(d_a), _ptr(d_b), _ptr(out), ctx.stream())
    return out


def lindell_ntilde_generate(ctx, count, seed, counter, max_attempts=0):
    """`party_one::generate_h1_h2_n_tilde()` x count (party_one.rs:594-607): dict of device tensors Nt, h1, h2 [count, 64], xhi [count, 8], fail [1]"""
    o = {f: _new(ctx, count, 64) for f in ("Nt", "h1", "h2")}
    o["xhi"] = _new(ctx, count, 8)
    fail = torch.zeros((1,), dtype=torch.int32, device=ctx.device)
    N_.call.mpe_lindell_ntilde_generate(ctx.h, count, _seed(seed), int(counter), max_attempts, _ptr(o["Nt"]), _ptr(o["h1"]), _ptr(o["h2"]), _ptr(o["xhi"]),
                                        _ptr(fail), ctx.stream())
    o["fail"] = fail
    return o


# stream fields of the three chains below (field f of a call draws stream counter | f << 56)
LINDELL_FIELDS = dict(x1=16, x2=17, blind_pk=18, blind_pok=19, nonce1=20, nonce2=21, enc_r=22, cdlog_r=23, pdl_alpha=24, pdl_beta=25, pdl_rho=26,
                      pdl_gamma=27, k1=32, k2=33, eph_nonce1=34, eph_nonce2=35, eph_blind_pk=36, eph_blind_pok=37)
LINDELL_MATERIAL_FIELDS = ("p", "q", "pt", "qt", "h1", "xhi")     # rows [B, 32] x 4, [B, 64], [B, 8]
_Q = 0xFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFEBAAEDCE6AF48A03BBFD25E8CD0364141


def _widen(t, words):
    out = torch.zeros((t.shape[0], words), dtype=torch.int32, device=t.device)
    out[:, :t.shape[1]] = t
    return out


def _lindell_paillier_half(ctx, B, seed, counter, d_x1, d_q1, material=None):
    """What lindell_keygen and lindell_rotate share: `generate_keypair_and_encrypted_share`, `generate_ni_proof_correct_key`,
    `verify_ni_proof_correct_key`, `pdl_proof`, `pdl_verify` (party_one.rs:319-401, party_two.rs:275-311) for the shares d_x1 [B,8]
    (canonical scalars); d_q1 [B,16] is the Q1 party two holds.  One Paillier key and one (N~, h1, h2) per wallet."""
    sid = lambda f: int(counter) | (LINDELL_FIELDS[f] << 56)
    fails = []
    if material is None:
        p, q, N, f = paillier_keygen(ctx, B, seed, counter)
        nt = lindell_ntilde_generate(ctx, B, seed, counter)
        Nt, h1, h2, xhi = nt["Nt"], nt["h1"], nt["h2"], nt["xhi"]
        fails += [f, nt["fail"]]
    else:
        m = {f: words_to_ints(np.ascontiguousarray(material[f])) for f in LINDELL_MATERIAL_FIELDS}
        if any(len(v) != B for v in m.values()):
            raise ValueError("material: B rows per field")
        nts = [a * b for a, b in zip(m["pt"], m["qt"])]
        p, q, N = dev(ctx, m["p"], 32), dev(ctx, m["q"], 32), dev(ctx, [a * b for a, b in zip(m["p"], m["q"])], 64)
        Nt, h1, xhi = dev(ctx, nts, 64), dev(ctx, m["h1"], 64), dev(ctx, m["xhi"], 8)
        h2 = dev(ctx, [pow(pow(h, -1, n), x, n) for h, x, n in zip(m["h1"], m["xhi"], nts)], 64)
    ctx.sync()
    Ni, Nti = host(N), host(Nt)                                  # public moduli: the sampler's bounds are formed from them on the host
    sk = PaillierKeys(ctx, p=p, q=q)
    pk = PaillierKeys(ctx, N=Ni)                                 # what party two holds
    r, f = sample_below(ctx, B, seed, sid("enc_r"), N, 64)       # Randomness::sample(&ek)
    fails.append(f)
    c_key = sk.encrypt_device(_widen(d_x1, 64), r)
    sigma = correct_key_prove(ctx, sk).reshape(B, 11 * 64)
    ok_ck = correct_key_verify(ctx, N, sigma)
    long_enough = ((N[:, 63].to(torch.int64) & 0xFFFFFFFF) >> 30) != 0     # ek.n.bit_length() >= PAILLIER_KEY_SIZE - 1 (party_two.rs:307)
    # pdl_proof (party_one.rs:366-401)
    cd_r = sample_bits(ctx, B, seed, sid("cdlog_r"), 512, 16)
    cd_x, cd_y = composite_dlog_prove(ctx, Nt, h1, h2, _widen(xhi, 64), cd_r)
    stm = Statements(ctx, Nt, h1, h2, wb=0)
    nonces = {}
    nonces["alpha"], f1 = sample_below(ctx, B, seed, sid("pdl_alpha"), dev(ctx, [_Q ** 3], 24), 24)
    nonces["beta"], f2 = sample_below(ctx, B, seed, sid("pdl_beta"), dev(ctx, [max(n - 2, 0) for n in Ni], 64), 64, flags=SAMPLE_PLUS_ONE)
    nonces["rho"], f3 = sample_below(ctx, B, seed, sid("pdl_rho"), dev(ctx, [_Q * n for n in Nti], 72), 72)
    nonces["gamma"], f4 = sample_below(ctx, B, seed, sid("pdl_gamma"), dev(ctx, [_Q ** 3 * n for n in Nti], 88), 88)
    fails += [f1, f2, f3, f4]
    Q, proof = lindell_pdl_proof(ctx, sk, stm, c_key, d_x1, r, nonces)
    ok_pdl = lindell_pdl_verify(ctx, pk, Nt, h1, h2, cd_x, cd_y, N, c_key, Q, c_key, d_q1, proof)
    ok = ok_ck.bool() & long_enough & ok_pdl.bool()
    ctx.sync()
    stm.close(); sk.close(); pk.close()
    return dict(ok=ok, fails=fails, p=p, q=q, N=N, c_key=c_key, r=r, Nt=Nt, h1=h1, h2=h2, xhi=xhi, sigma=sigma, cd_x=cd_x, cd_y=cd_y, Q=Q, pdl=proof)


def _given_scalars(ctx, v):
    """a share handed in: a device tensor [B,8] of canonical scalars, or Python ints (reduced mod q, as Scalar::from does)"""
    return v if torch.is_tensor(v) else dev(ctx, [int(x) % _Q for x in v], 8)


def lindell_keygen(ctx, B, seed, counter=0, x1=None, x2=None, material=None):
    """`test_full_key_gen` (lindell_2017/test.rs) for B wallets with both parties local: a chain of C-ABI calls, no secret on the host.
      x1 / x2:  None = drawn by the device sampler; given = the `_with_fixed_secret_share` forms.
      material: None = mint the Paillier key and (N~, h1, h2, xhi) on the device (streams counter | 0, 1, 6, 7, 14, 15 << 56); or a dict
                of uint32 arrays LINDELL_MATERIAL_FIELDS taken as `Paillier::keypair()` / `generate_h1_h2_n_tilde()` would have drawn them.
      Every other draw: streams counter | LINDELL_FIELDS[..] << 56 of `seed`.
    Returns a dict: ok [B] uint8 (both first-message verdicts, the correct-key and PDL verdicts, pubkeys agree), failures (sampler /
    prime search give-ups), the wallet x1, x2 [B,8], Q1, Q2, pubkey [B,16], p, q [B,32], N [B,64], c_key [B,128], r [B,64], and `proofs`."""
    if counter >> 56:
        raise ValueError("counter < 2^56")
    sid = lambda f: int(counter) | (LINDELL_FIELDS[f] << 56)
    fails = []

    def scalar(f):
        v, fl = sample_scalar(ctx, B, seed, sid(f))
        fails.append(fl)
        return v
    x1 = scalar("x1") if x1 is None else _given_scalars(ctx, x1)
    x2 = scalar("x2") if x2 is None else _given_scalars(ctx, x2)
    blind_pk, blind_pok = sample_bits(ctx, B, seed, sid("blind_pk"), 256, 8), sample_bits(ctx, B, seed, sid("blind_pok"), 256, 8)
    m1 = lindell_keygen_first_msg(ctx, x1, scalar("nonce1"), blind_pk, blind_pok)                      # party one
    Q2, R2, z2 = dlog_prove(ctx, x2, scalar("nonce2"))                                                   # party two: KeyGenFirstMsg::create
    ok_p1 = dlog_verify(ctx, Q2, R2, z2)                                                                 # party one: verify_and_decommit
    ok_p2 = lindell_keygen_verify_first_msg(ctx, m1["pk_com"], m1["pok_com"], blind_pk, blind_pok, m1["Q1"], m1["R"], m1["z"])
    half = _lindell_paillier_half(ctx, B, seed, counter, x1, m1["Q1"], material)
    pub1, pub2 = ec_mul(ctx, x1, Q2), ec_mul(ctx, x2, m1["Q1"])                                          # compute_pubkey on both sides
    ok = ok_p1.bool() & ok_p2.bool() & half["ok"] & (pub1 == pub2).all(1)
    ctx.sync()
    return dict(ok=ok.to(torch.uint8), failures=int(sum(int(f.item()) for f in fails + half["fails"])), x1=x1, x2=x2, Q1=m1["Q1"], Q2=Q2,
                pubkey=pub1, p=half["p"], q=half["q"], N=half["N"], c_key=half["c_key"], r=half["r"],
                proofs=dict(first_msg=m1, blind_pk=blind_pk, blind_pok=blind_pok, half=half))


def lindell_eph_exchange(ctx, B, seed, counter):
    """the ephemeral exchange both ways: party one's `EphKeyGenFirstMsg::create` (two base multiplications + mpe_ecddh_prove) checked by
    party two's `verify_and_decommit` (mpe_ecddh_verify), party two's `create_commitments` checked by party one's verdict.
    Returns dict ok [B] uint8, k1, k2 [B,8], R1, R2 [B,16] (what lindell_partial_sig / lindell_sign take), failures."""
    if counter >> 56:
        raise ValueError("counter < 2^56")
    sid = lambda f: int(counter) | (LINDELL_FIELDS[f] << 56)
    fails = []

    def scalar(f):
        v, fl = sample_scalar(ctx, B, seed, sid(f))
        fails.append(fl)
        return v
    k1, k2 = scalar("k1"), scalar("k2")
    blind_pk, blind_pok = sample_bits(ctx, B, seed, sid("eph_blind_pk"), 256, 8), sample_bits(ctx, B, seed, sid("eph_blind_pok"), 256, 8)
    Gp = dev(ctx, [0x79BE667EF9DCBBAC55A06295CE870B07029BFCDB2DCE28D959F2815B16F81798 |
                   (0x483ADA7726A3C4655DA4FBFC0E1108A8FD17B448A68554199C47D08FFB10D4B8 << 256)], 16).expand(B, 16).contiguous()
    Hp = dev(ctx, [0x08d13221e3a7326a34dd45214ba80116dd142e4b5ff3ce66a8dc7bfa0378b795 |
                   (0x5d41ac1477614b5c0848d50dbd565ea2807bcba1df0df07a8217e9f7f7c2be88 << 256)], 16).expand(B, 16).contiguous()
    R1 = ec_mul_base(ctx, k1)
    st1 = dict(g1=Gp, h1=R1, g2=Hp, h2=ec_mul(ctx, k1, Hp))
    pr1 = ecddh_prove(ctx, k1, scalar("eph_nonce1"), st1)
    ok_a = ecddh_verify(ctx, st1, pr1)
    m2 = lindell_eph_first_msg(ctx, k2, scalar("eph_nonce2"), blind_pk, blind_pok)
    ok_b = lindell_eph_verify_first_msg(ctx, m2["pk_com"], m2["pok_com"], blind_pk, blind_pok, m2["pub"], m2["c"], m2["a1"], m2["a2"], m2["z"])
    ok = ok_a.bool() & ok_b.bool()
    ctx.sync()
    return dict(ok=ok.to(torch.uint8), k1=k1, k2=k2, R1=R1, R2=m2["pub"], failures=int(sum(int(f.item()) for f in fails)),
                proofs=dict(p1=dict(st1, **pr1), p2=m2, blind_pk=blind_pk, blind_pok=blind_pok))


def lindell_rotate(ctx, wallet, d_factor, seed, counter, d_factor2=None, material=None):
    """`Party1Private::refresh_private_key(factor)` (party_one.rs:246-296): a new Paillier key, x1 f, a new c_key, the correct-key proof
    and the PDL triple, checked as party two checks them against f Q1 — the second half of lindell_keygen over another x1.
    d_factor2 given: `Party2Private::update_private_key` (party_two.rs:241-246), x2 <- x2 factor2.  Returns the new wallet dict (same
    fields as lindell_keygen's; pubkey is the OLD one, which still verifies when factor2 = factor^-1)."""
    B = wallet["x1"].shape[0]
    if counter >> 56:
        raise ValueError("counter < 2^56")
    x1 = scalar_mul(ctx, wallet["x1"], d_factor)
    q1 = ec_mul(ctx, d_factor, wallet["Q1"])
    half = _lindell_paillier_half(ctx, B, seed, counter, x1, q1, material)
    out = dict(wallet)
    out.update(ok=half["ok"].to(torch.uint8), failures=int(sum(int(f.item()) for f in half["fails"])), x1=x1, Q1=q1, p=half["p"], q=half["q"],
               N=half["N"], c_key=half["c_key"], r=half["r"], proofs=dict(half=half))
    if d_factor2 is not None:
        out["x2"] = scalar_mul(ctx, wallet["x2"], d_factor2)
        out["Q2"] = ec_mul(ctx, d_factor2, wallet["Q2"])
    ctx.sync()
    return out


# ================================================================================================
# GG18 threshold signing (mpe_gg18.h; gg_2018/party_i.rs:384-737, examples/gg18_sign_client.rs)
# ================================================================================================
def _g18_dims(signers, local):
    sg = (C.c_int32 * len(signers))(*[int(s) for s in signers])
    lc = (C.c_int32 * len(local))(*[int(x) for x in local])
    return len(signers), sg, len(local), lc


def gg18_sign_keys(ctx, t, n, signers, local, d_x_i, d_pk_vec, d_k_i, d_gamma_i):
    """`SignKeys::create`: x_i, k_i, gamma_i [L,B,8], pk_vec [B,n,16] -> dict w_i [L,B,8], g_w_i, g_gamma_i [L,B,16], g_w [S,B,16], status [L,B]"""
    L, B = d_k_i.shape[0], d_k_i.shape[1]
    S = len(signers)
    o = dict(w_i=_new(ctx, L, B, 8), g_w_i=_new(ctx, L, B, 16), g_gamma_i=_new(ctx, L, B, 16),
             g_w=_new(ctx, S, B, 16), status=torch.zeros((L, B), dtype=torch.int32, device=ctx.device))
    N_.call.mpe_gg18_sign_keys(ctx.h, t, n, *_g18_dims(signers, local), B, _ptr(d_x_i), _ptr(d_pk_vec), _ptr(d_k_i), _ptr(d_gamma_i), _ptr(o["w_i"]),
                               _ptr(o["g_w_i"]), _ptr(o["g_gamma_i"]), _ptr(o["g_w"]), _ptr(o["status"]), ctx.stream())
    return o


def gg18_message_b(ctx, pk, d_b, d_ca, d_r, d_beta_tag, d_nonce_b, d_nonce_bt, d_key_idx=None):
    """`MessageB::b_with_predefined_randomness(.., &[])`, flat items: returns dict(c, beta, b_proof, beta_tag_proof)"""
    B = d_b.shape[0]
    out = dict(c=_new(ctx, B, 128), beta=_new(ctx, B, 8), b_proof=dict(pk=_new(ctx, B, 16), R=_new(ctx, B, 16), z=_new(ctx, B, 8)),
               beta_tag_proof=dict(pk=_new(ctx, B, 16), R=_new(ctx, B, 16), z=_new(ctx, B, 8)))
    p1, p2 = _struct(N_.DlogProof, out["b_proof"]), _struct(N_.DlogProof, out["beta_tag_proof"])
    N_.call.mpe_gg18_message_b(ctx.h, pk.h, B, _ptr(d_key_idx), _ptr(d_b), _ptr(d_ca), _ptr(d_r), _ptr(d_beta_tag), _ptr(d_nonce_b), _ptr(d_nonce_bt),
                               _ptr(out["c"]), _ptr(out["beta"]), C.byref(p1), C.byref(p2), ctx.stream())
    return out


def gg18_phase2(ctx, signers, local, d_k_i, d_gamma_i, d_w_i, d_alpha, d_beta, d_miu, d_ni, d_ok_gamma, d_ok_w, d_w_pk, d_g_w, d_status):
    """the alpha verdicts (201 / 202), `phase2_delta_i`, `phase2_sigma_i`: per-peer inputs [L,S-1,B,..] -> (delta_i, sigma_i) [L,B,8]"""
    L, B = d_k_i.shape[0], d_k_i.shape[1]
    delta, sigma = _new(ctx, L, B, 8), _new(ctx, L, B, 8)
    N_.call.mpe_gg18_phase2(ctx.h, *_g18_dims(signers, local), B, _ptr(d_k_i), _ptr(d_gamma_i), _ptr(d_w_i), _ptr(d_alpha), _ptr(d_beta), _ptr(d_miu),
                            _ptr(d_ni), _ptr(d_ok_gamma), _ptr(d_ok_w), _ptr(d_w_pk), _ptr(d_g_w), _ptr(delta), _ptr(sigma), _ptr(d_status), ctx.stream())
    return delta, sigma


def gg18_phase4(ctx, signers, local, d_delta, d_b_pk, d_g_gamma, d_blind, d_com, d_status):
    """`phase3_reconstruct_delta` + `phase4` + the own g_gamma_i: broadcast [S,B,..], b_pk [L,S-1,B,16] -> R [L,B,16]"""
    L, B = d_status.shape
    R = _new(ctx, L, B, 16)
    N_.call.mpe_gg18_phase4(ctx.h, *_g18_dims(signers, local), B, _ptr(d_delta), _ptr(d_b_pk), _ptr(d_g_gamma), _ptr(d_blind), _ptr(d_com), _ptr(R),
                            _ptr(d_status), ctx.stream())
    return R


def gg18_phase5a(ctx, signers, local, d_k_i, d_sigma_i, d_msg, d_R, d_l_i, d_rho_i, d_blind, d_s1, d_s2, d_nonce, d_status):
    """`phase5_local_sig` + `phase5a_broadcast_5b_zkproof`: dict s_i, V, A, B, com, heg{T, A3, z1, z2}, dlog{pk, R, z}, all [L,B,..]"""
    L, B = d_status.shape
    new = lambda w: _new(ctx, L, B, w)
    o = dict(s_i=new(8), V=new(16), A=new(16), B=new(16), com=new(8), heg=dict(T=new(16), A3=new(16), z1=new(8), z2=new(8)),
             dlog=dict(pk=new(16), R=new(16), z=new(8)))
    hp, dp = _struct(N_.HegProof, o["heg"]), _struct(N_.DlogProof, o["dlog"])
    N_.call.mpe_gg18_phase5a(ctx.h, *_g18_dims(signers, local), B, _ptr(d_k_i), _ptr(d_sigma_i), _ptr(d_msg), _ptr(d_R), _ptr(d_l_i), _ptr(d_rho_i),
                             _ptr(d_blind), _ptr(d_s1), _ptr(d_s2), _ptr(d_nonce), _ptr(o["s_i"]), _ptr(o["V"]), _ptr(o["A"]), _ptr(o["B"]), _ptr(o["com"]),
                             C.byref(hp), C.byref(dp), _ptr(d_status), ctx.stream())
    return o


GG18_PHASE5B_FIELDS = ("V", "A", "B", "blind", "com", "T", "A3", "z1", "z2", "dlog_pk", "dlog_R", "dlog_z")


def gg18_phase5c(ctx, signers, local, d_msg, d_y, d_R, d_l_i, d_rho_i, d_blind2, bc, d_status):
    """`phase5c`: bc = dict GG18_PHASE5B_FIELDS of broadcast arrays [S,B,..] -> (u, t [L,B,16], com2 [L,B,8])"""
    L, B = d_status.shape
    u, t, com2 = _new(ctx, L, B, 16), _new(ctx, L, B, 16), _new(ctx, L, B, 8)
    st = _struct(N_.Gg18Phase5bMsgs, bc)
    N_.call.mpe_gg18_phase5c(ctx.h, *_g18_dims(signers, local), B, _ptr(d_msg), _ptr(d_y), _ptr(d_R), _ptr(d_l_i), _ptr(d_rho_i), _ptr(d_blind2), C.byref(st),
                             _ptr(u), _ptr(t), _ptr(com2), _ptr(d_status), ctx.stream())
    return u, t, com2


def gg18_phase5d(ctx, signers, local, d_u, d_t, d_blind2, d_com2, d_B, d_status):
    """`phase5d` over the broadcast arrays [S,B,..]: writes 541 / 542 into d_status"""
    B = d_status.shape[1]
    N_.call.mpe_gg18_phase5d(ctx.h, *_g18_dims(signers, local), B, _ptr(d_u), _ptr(d_t), _ptr(d_blind2), _ptr(d_com2), _ptr(d_B), _ptr(d_status), ctx.stream())


def gg18_output_signature(ctx, signers, local, d_s_own, d_s_all, d_R, d_msg, d_y, d_status):
    """`output_signature`: s_own, R [L,B,..], s_all [S,B,8] -> (r, s [L,B,8], recid [L,B]); zero unless the status is 0"""
    L, B = d_status.shape
    r, s = _new(ctx, L, B, 8), _new(ctx, L, B, 8)
    recid = torch.zeros((L, B), dtype=torch.int32, device=ctx.device)
    N_.call.mpe_gg18_output_signature(ctx.h, *_g18_dims(signers, local), B, _ptr(d_s_own), _ptr(d_s_all), _ptr(d_R), _ptr(d_msg), _ptr(d_y), _ptr(r), _ptr(s),
                                      _ptr(recid), _ptr(d_status), ctx.stream())
    return r, s, recid


class Gg18Wallet(_Handle):
    """What GG18 signing reads of a `LocalKey`, resident in HBM, in the shape Gg20Keys takes it: arrays = dict of numpy uint32 arrays over
    ALL n parties: x [n,8], p, q [n,32], X [n,16] (pk_vec), y [1,16], optionally N [n,64] (else p q).  own: the party indices whose
    secrets (x, p, q) this object gets (default all); the other parties' rows of x, p, q never leave the host."""
    pk = sk = None

    def __init__(self, ctx, t, n, arrays, own=None):
        self.ctx, self.t, self.n = ctx, t, n
        self.own = list(range(n)) if own is None else sorted(int(a) for a in own)
        a = {f: np.ascontiguousarray(arrays[f]) for f in ("x", "p", "q", "X", "y")}
        if arrays.get("N") is not None:
            Nw = np.ascontiguousarray(arrays["N"])
        else:
            Nw = ints_to_words([p_ * q_ for p_, q_ in zip(words_to_ints(a["p"]), words_to_ints(a["q"]))], 64)
        up = lambda v: torch.from_numpy(np.ascontiguousarray(v).view(np.int32)).to(ctx.device)
        self.x, self.X, self.y, self.N = up(a["x"][self.own]), up(a["X"][:n]), up(a["y"][:1]), up(Nw[:n])
        self.pk = PaillierKeys(ctx, N=words_to_ints(Nw[:n]))                        # every party's public key
        self.sk = PaillierKeys(ctx, p=up(a["p"][self.own]), q=up(a["q"][self.own]))  # the own ones, in the order of `own`

    def close(self):                          # no handle of its own: the two key sets
        for keys in (self.pk, self.sk):
            if keys is not None:
                keys.close()


# stream fields of gg18_sign (field f draws stream counter | f << 56; 0..21 are mpe_gg20_sample_nonces', 0..15 the keygen chains',
# 16..37 LINDELL_FIELDS)
GG18_FIELDS = dict(k=40, gamma=41, blind=42, r_a=43, mb_beta_tag=44, mb_r=45, mb_nonce_b=46, mb_nonce_bt=47, l=48, rho=49, blind5a=50, heg_s1=51,
                   heg_s2=52, dlog_nonce=53, blind5c=54)
# messages of the nine broadcast / P2P rounds of gg18_sign_client.rs: field -> (round, words); every array is sender-major [S, B, w], the
# MessageB fields [S, S-1, 2, B, w] (peer slot, then 0 = gamma side / 1 = w side)
GG18_MSG_FIELDS = dict(com=(1, 8), c_a=(1, 128), mb_c=(2, 128), mb_b_pk=(2, 16), mb_b_R=(2, 16), mb_b_z=(2, 8), mb_bt_pk=(2, 16), mb_bt_R=(2, 16),
                       mb_bt_z=(2, 8), delta=(3, 8), blind=(4, 8), g_gamma=(4, 16), com5a=(5, 8), V=(6, 16), A=(6, 16), B=(6, 16), blind5a=(6, 8),
                       heg_T=(6, 16), heg_A3=(6, 16), heg_z1=(6, 8), heg_z2=(6, 8), dlog_pk=(6, 16), dlog_R=(6, 16), dlog_z=(6, 8), com5c=(7, 8),
                       u=(8, 16), t=(8, 16), blind5c=(8, 8), s_i=(9, 8))


def gg18_draw_shapes(S, L, B):
    """shape of every field of `draws`: per local party [L, B, w]; the MessageB fields [2, L, S-1, B, w] (side, party, peer slot)"""
    one = lambda w: (L, B, w)
    mb = lambda w: (2, L, S - 1, B, w)
    return dict(k=one(8), gamma=one(8), blind=one(8), r_a=one(64), mb_beta_tag=mb(64), mb_r=mb(64), mb_nonce_b=mb(8), mb_nonce_bt=mb(8), l=one(8),
                rho=one(8), blind5a=one(8), heg_s1=one(8), heg_s2=one(8), dlog_nonce=one(8), blind5c=one(8))


def gg18_sign(ctx, wallet, signers, d_msg, B, seed=None, counter=0, draws=None, local=None, _fault=None):
    """The ten rounds of examples/gg18_sign_client.rs for B sessions in lock step, one call per phase over all of its items:
    SignKeys | com + MessageA | MessageB x 2 per peer | alphas + delta_i / sigma_i | phase 4 | 5A | 5B | 5C | 5D | s_i + output.
      wallet:  Gg18Wallet; signers: party indices, ascending; d_msg: device [B,8] (the hashed messages); local: signer ordinals played
               here (default all).
      draws:   None = every value the reference takes from OsRng is drawn by the device sampler from (seed, counter): stream
               counter | GG18_FIELDS[f] << 56, rules sample_scalar, sample_bits(256) for the blind factors, sample_below(N_peer) for the
               Paillier randomness and beta_tag (N_own for r_a); or a dict of arrays gg18_draw_shapes that replaces the sampler.
      _fault:  a test aid, not part of the interface: _fault(round, msgs) is called when the messages of round 1..9 are in `msgs`
               (GG18_MSG_FIELDS, sender-major device tensors; msgs["draws"] is the draws dict) and may edit them in place — a peer's
               rows when `local` is a subset, a tampered value otherwise.
    Every party reads every broadcast value, its own included, from `msgs`; a party that has failed sends zero words from then on.
    Returns a dict: status [B, L] (include/mpecdsa_hip.h lists the codes), r, s [B,8], recid [B] of the first local party and
    r_all, s_all [L,B,8], recid_all [L,B], R [L,B,16], draws, msgs, failures (sampler give-ups).  No secret is copied to the host."""
    signers = [int(s) for s in signers]
    S, n = len(signers), wallet.n
    local = list(range(S)) if local is None else [int(x) for x in local]
    L, P1, dev_ = len(local), S - 1, ctx.device
    if counter >> 56:
        raise ValueError("counter < 2^56")
    own_pos = [wallet.own.index(signers[i]) for i in local]                    # rows of wallet.x / keys of wallet.sk
    ind = [[jj if jj < i else jj + 1 for jj in range(P1)] for i in local]       # peer ordinal of (local party, slot)
    jme = [[(i if i < ind[li][jj] else i - 1) for jj in range(P1)] for li, i in enumerate(local)]      # my slot at that peer
    it = lambda v: torch.tensor(v, dtype=torch.int64, device=dev_)
    i32 = lambda v: torch.tensor(v, dtype=torch.int32, device=dev_)
    t_loc, t_ind, t_jme = it(local), it(ind), it(jme)
    key_own = i32(own_pos).reshape(L, 1).expand(L, B).contiguous()                                      # [L,B] key of wallet.sk
    key_peer = i32([[signers[j] for j in row] for row in ind]).reshape(1, L, P1, 1).expand(2, L, P1, B).contiguous()   # key of wallet.pk
    fails = []
    if draws is None:
        sid = lambda f: int(counter) | (GG18_FIELDS[f] << 56)
        draws = {}

        def scalar(f, shape):
            v, fl = sample_scalar(ctx, int(np.prod(shape[:-1])), seed, sid(f))
            fails.append(fl)
            return v.reshape(shape)
        for f, shape in gg18_draw_shapes(S, L, B).items():
            rows = int(np.prod(shape[:-1]))
            if f in ("blind", "blind5a", "blind5c"):
                draws[f] = sample_bits(ctx, rows, seed, sid(f), 256, 8).reshape(shape)
            elif f == "r_a":                                                   # Randomness of MessageA::a: below the own N   mta/mod.rs:57
                own_N = i32([signers[i] for i in local]).reshape(L, 1).expand(L, B).contiguous()
                v, fl = sample_below(ctx, rows, seed, sid(f), wallet.N, 64, own_N.reshape(-1))
                fails.append(fl)
                draws[f] = v.reshape(shape)
            elif f in ("mb_beta_tag", "mb_r"):                                 # below the PEER's N                           mta/mod.rs:97-98
                v, fl = sample_below(ctx, rows, seed, sid(f), wallet.N, 64, key_peer.reshape(-1))
                fails.append(fl)
                draws[f] = v.reshape(shape)
            else:
                draws[f] = scalar(f, shape)
    else:
        shapes = gg18_draw_shapes(S, L, B)
        draws = {f: (v if torch.is_tensor(v) else _dev_u32(np.ascontiguousarray(v, dtype=np.uint32), dev_)).reshape(shapes[f]).contiguous()
                 for f, v in draws.items()}
    z = draws
    msgs = {f: torch.zeros((S, B, w) if not f.startswith("mb_") else (S, P1, 2, B, w), dtype=torch.int32, device=dev_)
            for f, (_, w) in GG18_MSG_FIELDS.items()}
    msgs["draws"] = draws
    hook = (lambda rnd: _fault(rnd, msgs)) if _fault is not None else (lambda rnd: None)

    def put(name, val, status):
        """the local parties' rows of a broadcast field; a failed party sends zero words"""
        alive = (status == 0).reshape(status.shape + (1,) * (val.dim() - 2)).to(val.dtype)
        msgs[name][t_loc] = val * alive

    y = wallet.y.expand(B, 16).contiguous()
    pk_vec = wallet.X.reshape(1, n, 16).expand(B, n, 16).contiguous()
    x_i = wallet.x[it(own_pos)].reshape(L, 1, 8).expand(L, B, 8).contiguous()
    # SignKeys::create (client :101-106)
    sk_ = gg18_sign_keys(ctx, wallet.t, n, signers, local, x_i, pk_vec, z["k"], z["gamma"])
    status, w_i, g_w = sk_["status"], sk_["w_i"], sk_["g_w"]
    # round 1: phase1_broadcast + MessageA::a(k_i, ek, &[]) (client :110-119)
    com = hash_commit_point(ctx, sk_["g_gamma_i"].reshape(L * B, 16), z["blind"].reshape(L * B, 8)).reshape(L, B, 8)
    c_a = wallet.sk.encrypt_device(_widen(z["k"].reshape(L * B, 8), 64), z["r_a"].reshape(L * B, 64), key_own.reshape(-1)).reshape(L, B, 128)
    put("com", com, status)
    put("c_a", c_a, status)
    hook(1)
    # round 2: MessageB::b(gamma_i | w_i, ek_peer, m_a_peer, &[]) toward every peer, ONE launch (client :151-195); items [2, L, S-1, B]
    nMB = 2 * L * P1 * B
    b_sel = torch.stack([z["gamma"], w_i]).reshape(2, L, 1, B, 8).expand(2, L, P1, B, 8).contiguous()
    ca_peer = msgs["c_a"][t_ind].reshape(1, L, P1, B, 128).expand(2, L, P1, B, 128).contiguous()
    mb = gg18_message_b(ctx, wallet.pk, b_sel.reshape(nMB, 8), ca_peer.reshape(nMB, 128), z["mb_r"].reshape(nMB, 64), z["mb_beta_tag"].reshape(nMB, 64),
                        z["mb_nonce_b"].reshape(nMB, 8), z["mb_nonce_bt"].reshape(nMB, 8), key_peer.reshape(-1))
    beta = mb["beta"].reshape(2, L, P1, B, 8)
    st_mb = status.reshape(L, 1, 1, B)
    for name, val in (("mb_c", mb["c"]), ("mb_b_pk", mb["b_proof"]["pk"]), ("mb_b_R", mb["b_proof"]["R"]), ("mb_b_z", mb["b_proof"]["z"]),
                      ("mb_bt_pk", mb["beta_tag_proof"]["pk"]), ("mb_bt_R", mb["beta_tag_proof"]["R"]), ("mb_bt_z", mb["beta_tag_proof"]["z"])):
        v = val.reshape(2, L, P1, B, -1).permute(1, 2, 0, 3, 4)                # [L, S-1, 2, B, w]: sender-major
        msgs[name][t_loc] = v * (st_mb == 0).reshape(L, 1, 1, B, 1).to(v.dtype)
    hook(2)
    # verify_proofs_get_alpha for both sides of every peer, ONE call (client :218-234), then delta_i / sigma_i (:246-247)
    recv = lambda name: msgs[name][t_ind, t_jme].permute(2, 0, 1, 3, 4).contiguous()          # [2, L, S-1, B, w]: what each peer sent ME
    rb = {f: recv("mb_b_" + f).reshape(nMB, -1) for f in ("pk", "R", "z")}
    rbt = {f: recv("mb_bt_" + f).reshape(nMB, -1) for f in ("pk", "R", "z")}
    a_it = z["k"].reshape(1, L, 1, B, 8).expand(2, L, P1, B, 8).contiguous().reshape(nMB, 8)
    key_it = key_own.reshape(1, L, 1, B).expand(2, L, P1, B).contiguous().reshape(-1)
    alpha, _share, ok = mta_verify_get_alpha(ctx, wallet.sk, recv("mb_c").reshape(nMB, 128), rb, rbt, a_it, key_it)
    alpha, ok, rpk = alpha.reshape(2, L, P1, B, 8), ok.reshape(2, L, P1, B), rb["pk"].reshape(2, L, P1, B, 16)
    delta_i, sigma_i = gg18_phase2(ctx, signers, local, z["k"], z["gamma"], w_i, alpha[0].contiguous(), beta[0].contiguous(), alpha[1].contiguous(),
                                   beta[1].contiguous(), ok[0].contiguous(), ok[1].contiguous(), rpk[1].contiguous(), g_w, status)
    del _share
    put("delta", delta_i, status)
    hook(3)
    # round 4: the decommitment, then phase3_reconstruct_delta + phase4 (client :272-309)
    put("blind", z["blind"], status)
    put("g_gamma", sk_["g_gamma_i"], status)
    hook(4)
    R = gg18_phase4(ctx, signers, local, msgs["delta"], rpk[0].contiguous(), msgs["g_gamma"], msgs["blind"], msgs["com"], status)
    # 5A, 5B (client :313-378)
    a5 = gg18_phase5a(ctx, signers, local, z["k"], sigma_i, d_msg, R, z["l"], z["rho"], z["blind5a"], z["heg_s1"], z["heg_s2"], z["dlog_nonce"], status)
    put("com5a", a5["com"], status)
    hook(5)
    for name, val in (("V", a5["V"]), ("A", a5["A"]), ("B", a5["B"]), ("blind5a", z["blind5a"]), ("heg_T", a5["heg"]["T"]), ("heg_A3", a5["heg"]["A3"]),
                      ("heg_z1", a5["heg"]["z1"]), ("heg_z2", a5["heg"]["z2"]), ("dlog_pk", a5["dlog"]["pk"]), ("dlog_R", a5["dlog"]["R"]),
                      ("dlog_z", a5["dlog"]["z"])):
        put(name, val, status)
    hook(6)
    # 5C (client :379-427)
    bc = dict(V=msgs["V"], A=msgs["A"], B=msgs["B"], blind=msgs["blind5a"], com=msgs["com5a"], T=msgs["heg_T"], A3=msgs["heg_A3"], z1=msgs["heg_z1"],
              z2=msgs["heg_z2"], dlog_pk=msgs["dlog_pk"], dlog_R=msgs["dlog_R"], dlog_z=msgs["dlog_z"])
    u, t_, com5c = gg18_phase5c(ctx, signers, local, d_msg, y, R, z["l"], z["rho"], z["blind5c"], bc, status)
    put("com5c", com5c, status)
    hook(7)
    put("u", u, status)
    put("t", t_, status)
    put("blind5c", z["blind5c"], status)
    hook(8)
    # 5D, then the s_i and output_signature (client :455-488)
    gg18_phase5d(ctx, signers, local, msgs["u"], msgs["t"], msgs["blind5c"], msgs["com5c"], msgs["B"], status)
    put("s_i", a5["s_i"], status)
    hook(9)
    r, s, recid = gg18_output_signature(ctx, signers, local, a5["s_i"], msgs["s_i"], R, d_msg, y, status)
    ctx.sync()
    return dict(status=status.transpose(0, 1).contiguous(), r=r[0], s=s[0], recid=recid[0], r_all=r, s_all=s, recid_all=recid, R=R, draws=draws,
                msgs={f: v for f, v in msgs.items() if f != "draws"}, failures=int(sum(int(f.item()) for f in fails)))
