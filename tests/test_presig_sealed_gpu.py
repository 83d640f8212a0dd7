"""GPU tests of sealed presignature records (`mpe_gg20_sealed_presig_export` / `_import`; PresigPool.export / import_ with
`wrap=`).  (t, n) = (1, 3), 8 sessions, the same nonces run three times: (a) signed online directly; (b) exported sealed, the
pool thrown away, the sealed rows imported into other slots of a new pool in shuffled order and signed there — the same
(r, s, recid); (c) exported in the clear, so that the sealed bytes of (b) can be compared with tests/pyref_seal.py applied to
the plain record, which tests/pyref_presig.py restates.  Then the refusals (a tampered row, a row under another key, a slot that is
not empty) and the hygiene of the stage the clear records pass through."""
import numpy as np
import pytest
import torch

import fixtures as F
import gg20_fixture as G
import pyref_presig as PP
import pyref_seal as PS
import seal_cases as SC

pytestmark = pytest.mark.gpu

CAP, B, S = 70, 8, 2
SIGNERS = [0, 2]
NONCE_HI = 0x0F1E2D3C4B5A6978


def _dev(ctx, arr):
    return torch.from_numpy(np.ascontiguousarray(arr).view(np.int32)).to(ctx.device)


def _u32(t):
    return t.cpu().numpy().view(np.uint32)


def _i32(t):
    return t.cpu().numpy()


class World:
    def __init__(self, keys):
        from multi_party_ecdsa_amd import engine as E
        self.ctx = E.Context(0)                                           # its own context: the scratch audit below counts every buffer of it
        self.lk = G.make_local_keys(keys, 1, 3, SIGNERS)
        self.gk = E.Gg20Keys(self.ctx, 1, 3, SIGNERS, self.lk["arrays"])
        self.nonces = G.make_nonces(self.lk, B, seed="presig-sealed")
        self.dn = {f: _dev(self.ctx, v) for f, v in self.nonces.items()}
        self.wk, self.wk_other = E.WrapKey(self.ctx, SC.KEY), E.WrapKey(self.ctx, SC.OTHER_KEY)
        self.y = self.lk["arrays"]["y"][0]

    def pool(self):
        from multi_party_ecdsa_amd import engine as E
        return E.PresigPool(self.ctx, self.gk, [0, 1], CAP)

    def presign(self, pool):
        from multi_party_ecdsa_amd import engine as E
        slots = E.gg20_presign(self.ctx, self.gk, self.dn, B, pool)
        assert (slots >= 0).all() and not pool.last_status.any()
        return slots

    def close(self):
        for o in (self.wk, self.wk_other, self.gk, self.ctx):
            o.close()


@pytest.fixture(scope="module")
def w(keys):
    world = World(keys)
    yield world
    world.close()


@pytest.fixture(scope="module")
def runs(w):
    """(a) the direct signatures; (b) the sealed rows [B, 102]; (c) the clear records [B, 92] — all from the same nonces"""
    pool = w.pool()
    slots = w.presign(pool)
    r, s, recid, status = pool.sign_online(slots, w.dn["msg"])
    direct = dict(r=_u32(r).copy(), s=_u32(s).copy(), recid=_i32(recid).copy(), status=_i32(status).copy())
    slots = w.presign(pool)
    sealed, st = pool.export(slots, wrap=w.wk, nonce_hi=NONCE_HI)
    assert not _i32(st).any() and pool.audit() == dict(EMPTY=CAP, READY=0, SIGNED=0, BUSY=0, stray=0) and pool.free_slots() == CAP
    sealed = _u32(sealed).copy()
    slots = w.presign(pool)
    clear, st = pool.export(slots)
    assert not _i32(st).any()
    pool.close()                                                          # the pool's view is gone: the rows are the only copies
    return direct, sealed, _u32(clear).copy()


def test_sealed_rows_are_the_restatement_of_the_plain_record(w, runs):
    direct, sealed, clear = runs
    assert sealed.shape == (B, 28 + 32 * S + 10) and clear.shape == (B, 28 + 32 * S)
    ref = PP.Pool(SIGNERS, [0, 1], [w.lk["y"]], CAP)
    for g in range(B):
        rec = [int(x) for x in clear[g]]
        u = PP.record_unpack(rec)
        assert ref.record_ok(rec) and PP.record_pack(ref.mask, ref.local, 0, w.lk["y"], u["parties"]) == rec
        assert [p["k"] for p in u["parties"]] == [F.ints(w.nonces["k"][g * S + i:g * S + i + 1])[0] for i in range(S)]
        assert [int(x) for x in sealed[g]] == PS.seal_row(SC.KEY, PS.KIND_PRESIG, g, NONCE_HI, rec), g
        assert PS.unseal_row(SC.KEY, PS.KIND_PRESIG, len(rec), sealed[g]) == (0, rec)
    assert not (sealed[:, PS.HEAD:PS.HEAD + clear.shape[1]] == clear).all(axis=1).any()


def test_sealed_round_trip_signs_what_the_direct_path_signs(w, runs):
    import ossl
    direct, sealed, clear = runs
    assert not direct["status"].any() and ossl.ecdsa_verify(w.y, w.nonces["msg"], direct["r"], direct["s"]).all()
    pool = w.pool()
    assert pool.sealed_words == pool.record_words + 10 == sealed.shape[1]
    order = np.random.default_rng(4).permutation(B)
    there = np.array([(23 * i + 40) % CAP for i in range(B)], dtype=np.int32)      # other slots, both workgroups
    got = pool.import_(_dev(w.ctx, sealed[order]), there, wrap=w.wk)
    assert np.array_equal(got, there) and not pool.last_status.any()
    assert pool.audit() == dict(EMPTY=CAP - B, READY=B, SIGNED=0, BUSY=0, stray=0)
    r, s, recid, status = pool.sign_online(there, _dev(w.ctx, w.nonces["msg"][order]))
    assert not _i32(status).any()
    assert np.array_equal(_u32(r), direct["r"][order]) and np.array_equal(_u32(s), direct["s"][order]) and np.array_equal(_i32(recid), direct["recid"][order])
    assert ossl.ecdsa_verify(w.y, w.nonces["msg"][order], _u32(r), _u32(s)).all()
    assert pool.audit() == dict(EMPTY=CAP, READY=0, SIGNED=0, BUSY=0, stray=0)
    pool.close()


def test_tampered_row_other_key_and_occupied_slot(w, runs):
    direct, sealed, clear = runs
    pool = w.pool()
    assert list(pool.import_(_dev(w.ctx, sealed[:1]), [5], wrap=w.wk)) == [5]
    tampered = sealed[1].copy()
    tampered[PS.HEAD + 30] ^= np.uint32(1)                                # one bit of party 0's k_i
    foreign = np.array(PS.seal_row(SC.OTHER_KEY, PS.KIND_PRESIG, 2, NONCE_HI, clear[2]), dtype=np.uint32)      # authentic, under another wallet's key
    rows = np.stack([tampered, foreign, sealed[3]])
    assert list(pool.import_(_dev(w.ctx, rows), [6, 66, 5], wrap=w.wk)) == [-1] * 3
    assert list(pool.last_status) == [PS.REFUSED, PS.REFUSED, PP.IMPORT_NOT_EMPTY]
    assert pool.audit() == dict(EMPTY=CAP - 1, READY=1, SIGNED=0, BUSY=0, stray=0) and pool.free_slots() == CAP - 1
    # the foreign row is a good record under ITS key; an authentic row with a record of another pool is judged by import's own rules
    assert list(pool.import_(_dev(w.ctx, foreign[None]), [66], wrap=w.wk_other)) == [66]
    alien = clear[4].copy()
    alien[1] = 0b011                                                      # a signer-set mask that is none of the key object's
    alien_row = np.array(PS.seal_row(SC.KEY, PS.KIND_PRESIG, 0, NONCE_HI + 1, alien), dtype=np.uint32)
    assert list(pool.import_(_dev(w.ctx, alien_row[None]), [7], wrap=w.wk)) == [-1] and list(pool.last_status) == [PP.IMPORT_REFUSED]
    far = np.array([CAP, -1], dtype=np.int32)                             # out of range: 831 and an all-zero sealed row
    out, st = pool.export(far, wrap=w.wk, nonce_hi=NONCE_HI + 2)
    assert list(_i32(st)) == [PP.RECORD_RANGE] * 2 and not _u32(out).any()
    out, st = pool.export([8], wrap=w.wk, nonce_hi=NONCE_HI + 3)          # an EMPTY slot: 833
    assert list(_i32(st)) == [PP.EXPORT_NOT_READY] and not _u32(out).any()
    assert pool.audit() == dict(EMPTY=CAP - 2, READY=2, SIGNED=0, BUSY=0, stray=0)
    pool.close()


def test_the_stage_of_the_clear_records_is_zero_after_the_calls(w, runs):
    direct, sealed, clear = runs
    pool = w.pool()
    w.ctx.wipe()
    assert w.ctx.scratch_audit()[0] == 0
    assert list(pool.import_(_dev(w.ctx, sealed), list(range(B)), wrap=w.wk)) == list(range(B))
    nz, total = w.ctx.scratch_audit()
    assert nz == 0 and total >= B * clear.shape[1] * 4                    # the stage is one of the regions the audit counts
    out, st = pool.export(list(range(B)), wrap=w.wk, nonce_hi=NONCE_HI + 4)
    assert not _i32(st).any() and w.ctx.scratch_audit()[0] == 0
    # the very records, under the fresh nonce
    for g in range(B):
        assert [int(x) for x in _u32(out)[g]] == PS.seal_row(SC.KEY, PS.KIND_PRESIG, g, NONCE_HI + 4, clear[g])
    assert pool.audit() == dict(EMPTY=CAP, READY=0, SIGNED=0, BUSY=0, stray=0)
    pool.close()
