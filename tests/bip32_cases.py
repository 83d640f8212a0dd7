"""The case table of mpe_bip32_derive, shared by the CPU and GPU tests: 64 rows over two parents, depths 0 .. MAX_DEPTH in one batch.
The rows with a property of the CHILD (a leading zero byte in x, an even or an odd y) are searched for here, on the CPU, with the
restatement of tests/pyref_bip32.py; every expectation is that restatement's word."""
import functools

import fixtures as F
import pyref
import pyref_bip32 as PB

MAX_DEPTH = 5
ROWS = 64
TOP = (1 << 31) - 1              # the largest non-hardened index


def parents():
    """two parents whose private keys the CPU test knows: [(x, K = x G, chain code)]"""
    r = F.Rng("bip32-parents")
    out = []
    for _ in range(2):
        x = r.below(pyref.Q - 1) + 1
        out.append((x, pyref.ec_mul(x, pyref.G), r.bits(256).to_bytes(32, "big")))
    return out


def _search(parent, what):
    """the smallest index whose child of `parent` has the property"""
    _, K, cc = parent
    for i in range(1 << 16):
        step = PB.ckd_pub(K, cc, i)
        if step is not None and what(step[1]):
            return i
    raise AssertionError("no such child among 65 536 indices")


@functools.lru_cache(maxsize=None)
def table():
    """(parents, rows, names): rows = [dict(parent, path [MAX_DEPTH], depth)], names = {property: row}"""
    ps = parents()
    r = F.Rng("bip32-rows")
    idx = lambda: r.below(1 << 31)
    pad = lambda path: list(path) + [0] * (MAX_DEPTH - len(path))
    rows, names = [], {}

    def add(name, parent, path, depth=None):
        names[name] = len(rows)
        rows.append(dict(parent=parent, path=pad(path), depth=len(path) if depth is None else depth))
    # a child whose x has a leading zero byte is the PARENT of the next level: serP must still be 33 bytes
    add("leading zero byte", 0, [_search(ps[0], lambda c: c[0] >> 248 == 0), 7])
    add("even y", 1, [_search(ps[1], lambda c: c[1] & 1 == 0), idx()])
    add("odd y", 1, [_search(ps[1], lambda c: c[1] & 1 == 1), idx()])
    add("index 0", 0, [0])
    add("index 0 below", 1, [idx(), 0, 0])
    add("index 2^31 - 1", 0, [TOP])
    add("index 2^31 - 1 below", 1, [idx(), TOP, idx(), TOP])
    add("depth 0", 1, [])
    add("full depth", 0, [idx() for _ in range(MAX_DEPTH)])
    # the refused rows, each between sound neighbours
    add("hardened", 0, [1 << 31])
    add("after hardened", 0, [idx(), idx()])
    add("hardened below", 1, [idx(), idx(), (1 << 31) + 5, idx()])
    add("after hardened below", 1, [idx()])
    add("hardened beyond the depth", 0, [idx(), 0xFFFFFFFF], depth=1)          # an index the row never walks: sound
    add("over-deep", 0, [idx() for _ in range(MAX_DEPTH)], depth=MAX_DEPTH + 1)
    add("after over-deep", 1, [idx(), idx(), idx()])
    add("negative depth", 1, [idx()], depth=-1)
    add("bad parent index", 2, [idx()])
    add("negative parent index", -1, [idx()])
    add("after bad parent index", 0, [idx(), idx()])
    while len(rows) < ROWS:                       # every depth, both parents
        d = len(rows) % (MAX_DEPTH + 1)
        rows.append(dict(parent=(len(rows) // (MAX_DEPTH + 1)) % 2, path=pad([idx() for _ in range(d)]), depth=d))
    return ps, rows, names


def expected():
    """[(status, tweak, child or None, chain code)] of every row"""
    ps, rows, _ = table()
    pub = [(K, cc) for _, K, cc in ps]
    return [PB.derive(pub, rw["parent"], rw["path"], rw["depth"], MAX_DEPTH) for rw in rows]
