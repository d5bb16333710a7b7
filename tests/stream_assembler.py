"""Assemble HIMG streams by hand: any tree, any token sequence, any tables, any chunk order that the
format (as oracle/himg_oracle.c states it) allows -- including everything no encoder would write.

Test infrastructure only.

A tree is an int (a leaf: the nine-bit symbol) or a pair (a, b) of trees.  It is serialised in pre-order:
one 0 bit for a branch, a 1 bit and the nine symbol bits (LSB first) for a leaf, child a first.  Codes
follow from the shape: the root's code is empty, child a appends a 0 bit and child b a 1 bit, and the
stream carries a code's first bit first (LSB-first in every byte).

Tokens are (symbol, extra) pairs: a list of pairs or an (n, 2) integer array.  Symbols 0..255 are
literal bytes, 256 stands for two zeros, 257..260 for 3 + extra (2 bits), 7 + extra (4), 23 + extra (8)
and 279 + extra (14) zeros.
"""
import numpy as np

TWO, UP6, UP22, UP278, UP16662 = 256, 257, 258, 259, 260
RUN_BASE = {TWO: 2, UP6: 3, UP22: 7, UP278: 23, UP16662: 279}
RUN_BITS = {TWO: 0, UP6: 2, UP22: 4, UP278: 8, UP16662: 14}
MAX_RUN = 16662
_EXTRA_BITS = np.zeros(512, np.int64)
_RUN_LEN = np.ones(512, np.int64)
for _s in RUN_BASE:
    _EXTRA_BITS[_s] = RUN_BITS[_s]
    _RUN_LEN[_s] = RUN_BASE[_s]

KNOWN_TAGS = (b"FRMT", b"LMAP", b"LRES", b"QCFG", b"FMAP", b"FRES")


# ---- trees ------------------------------------------------------------------------------------------

def is_leaf(t):
    return isinstance(t, (int, np.integer))


def leaves(tree):
    """[(symbol, code length, code)] of every leaf, in the order the stream stores them."""
    out = []
    stack = [(tree, 0, 0)]
    while stack:
        t, n, code = stack.pop()
        if is_leaf(t):
            out.append((int(t), n, code))
        else:
            stack.append((t[1], n + 1, code | (1 << n)))
            stack.append((t[0], n + 1, code))
    return out


def depth(tree):
    return max(n for _, n, _ in leaves(tree))


def tree_bits(tree):
    """The serialised tree, one bit per element."""
    bits = []
    stack = [tree]
    while stack:
        t = stack.pop()
        if is_leaf(t):
            bits.append(1)
            bits.extend((int(t) >> k) & 1 for k in range(9))
        else:
            bits.append(0)
            stack.append(t[1])
            stack.append(t[0])
    return np.array(bits, np.uint8)


def tree_bytes(tree):
    return np.packbits(tree_bits(tree), bitorder="little")


def tree_from_codes(length, code):
    """The tree of a code table (length[s] == 0: symbol s has no code), as the encoder's trace gives it."""
    root = [None, None]
    for s in range(len(length)):
        n, c = int(length[s]), int(code[s])
        if n == 0:
            continue
        node = root
        for k in range(n - 1):
            b = (c >> k) & 1
            if node[b] is None:
                node[b] = [None, None]
            node = node[b]
        assert node[(c >> (n - 1)) & 1] is None
        node[(c >> (n - 1)) & 1] = s

    def freeze(t):
        if not isinstance(t, list):
            assert t is not None, "the code table leaves a branch without a child"
            return t
        return (freeze(t[0]), freeze(t[1]))
    if root[1] is None and is_leaf(root[0]):
        return root[0]     # a single symbol: the encoder stores one leaf and writes one-bit codes
    return freeze(root)


def balanced(symbols):
    """Depths differ by at most one; the symbols from left to right."""
    symbols = list(symbols)
    if len(symbols) == 1:
        return symbols[0]
    h = (len(symbols) + 1) // 2
    return (balanced(symbols[:h]), balanced(symbols[h:]))


def comb(symbols, deep_first=False):
    """A leaf and a deeper comb at every level: len(symbols) - 1 deep.  deep_first: the FIRST symbols get
    the longest codes."""
    symbols = list(symbols)
    if deep_first:
        symbols = symbols[::-1]
    t = symbols[-1]
    for k in range(len(symbols) - 2, -1, -1):
        t = (symbols[k], t) if k % 2 else (t, symbols[k])
    return t


def fixed_length(symbols, bits):
    """Every code exactly `bits` long: 2 ** bits leaves, the symbols repeated to fill them."""
    symbols = list(symbols)
    assert 1 <= len(symbols) <= 1 << bits
    return balanced([symbols[k % len(symbols)] for k in range(1 << bits)])


def chains(top_bits, n_chains, chain_to, tail_depth, symbols):
    """A complete tree of top_bits levels; n_chains of its 2 ** top_bits places carry a comb that reaches
    a branch at depth chain_to and goes tail_depth levels below it, the others a leaf.  With chain_to =
    11 every chain is an 11-bit prefix with a sub-tree tail_depth deep.  symbols: consumed left to right."""
    it = iter(symbols)
    places = []
    for k in range(1 << top_bits):
        if k < n_chains:
            places.append(comb([next(it) for _ in range(chain_to - top_bits + tail_depth + 1)]))
        else:
            places.append(next(it))

    def build(lo, hi):
        if hi - lo == 1:
            return places[lo]
        return (build(lo, (lo + hi) // 2), build((lo + hi) // 2, hi))
    return build(0, len(places))


# ---- tokens -----------------------------------------------------------------------------------------

def as_tokens(tokens):
    """(n, 3): symbol, extra, which of the symbol's leaves carries it (a third column is optional)."""
    t = np.asarray(tokens, np.int64)
    if t.ndim != 2:
        t = t.reshape(-1, 2)
    if t.shape[1] == 2:
        t = np.concatenate((t, np.zeros((t.shape[0], 1), np.int64)), 1)
    assert t.shape[1] == 3
    return t


def tokens_length(tokens):
    """Bytes the tokens decode to."""
    t = as_tokens(tokens)
    return int(np.where(t[:, 0] > 255, _RUN_LEN[t[:, 0]] + np.where(t[:, 0] > TWO, t[:, 1], 0), 1).sum())


def expand_tokens(tokens):
    t = as_tokens(tokens)
    n = np.where(t[:, 0] > 255, _RUN_LEN[t[:, 0]] + np.where(t[:, 0] > TWO, t[:, 1], 0), 1)
    return np.repeat(np.where(t[:, 0] > 255, 0, t[:, 0]).astype(np.uint8), n)


def run_token(zeros):
    """The encoder's token for a run of 1..16662 zeros."""
    assert 1 <= zeros <= MAX_RUN
    if zeros == 1:
        return (0, 0)
    if zeros == 2:
        return (TWO, 0)
    for s in (UP6, UP22, UP278, UP16662):
        if zeros < RUN_BASE[s] + (1 << RUN_BITS[s]):
            return (s, zeros - RUN_BASE[s])


def _runs(row):
    """(start, length) of every maximal zero run."""
    z = np.concatenate(([0], (np.asarray(row) == 0).astype(np.int8), [0]))
    d = np.diff(z)
    start = np.flatnonzero(d == 1)
    return start, np.flatnonzero(d == -1) - start


def _merge(row, run_pos, run_tok):
    """Literals of the row and the run tokens (position, symbol, extra), in stream order."""
    row = np.asarray(row)
    lit = np.flatnonzero(row != 0)
    pos = np.concatenate((lit, np.asarray(run_pos, np.int64)))
    tok = np.concatenate((np.stack((row[lit].astype(np.int64), np.zeros(lit.size, np.int64)), 1),
                          np.asarray(run_tok, np.int64).reshape(-1, 2)))
    return tok[np.argsort(pos, kind="stable")]


def encoder_tokens(row):
    """The reference's greedy rule: a maximal run, cut only every 16 662 zeros."""
    start, length = _runs(row)
    pos, tok = [], []
    for s, n in zip(start.tolist(), length.tolist()):
        while n > 0:
            k = min(n, MAX_RUN)
            pos.append(s)
            tok.append(run_token(k))
            s += k
            n -= k
    return _merge(row, pos, tok)


def split_tokens(row, rng, mode="random", have=None):
    """A legal split of every zero run that the greedy rule would not choose (have: the symbols that the
    tree has leaves for; None: all).
    mode "literal": literal zeros only; "random": pieces of random length, each as a run token or as
    literal zeros; "base": as many pieces with extra = 0 (3, 7, 23, 279 zeros) as fit."""
    start, length = _runs(row)
    pos, tok = [], []
    for s, n in zip(start.tolist(), length.tolist()):
        while n > 0:
            if mode == "literal":
                k = 1
            elif mode == "base":
                k = max(b for b in (1, 2, 3, 7, 23, 279) if b <= n)
            else:
                k = int(min(n, rng.choice((1, 1, 2, 3, 6, 7, 22, 23, 278, 279, int(rng.integers(1, MAX_RUN + 1))))))
            if have is not None and run_token(k)[0] not in have:
                k = 1 if 0 in have else max(b for b in range(1, n + 1) if run_token(b)[0] in have)
            if mode == "random" and k > 1 and rng.integers(4) == 0 and (have is None or 0 in have):
                for j in range(min(k, 4)):
                    pos.append(s + j)
                    tok.append((0, 0))
                k = min(k, 4)
            else:
                pos.append(s)
                tok.append(run_token(k))
            s += k
            n -= k
    return _merge(row, pos, tok)


def _code_tables(tree, root_leaf_bits):
    """(length[which][symbol], code[which][symbol], leaf index[which][symbol], has a leaf[symbol])."""
    by_sym = {}
    for k, (s, n, c) in enumerate(leaves(tree)):
        by_sym.setdefault(s, []).append((root_leaf_bits if is_leaf(tree) else n, c, k))
    assert max(n for v in by_sym.values() for n, _, _ in v) + 14 <= 62
    ndup = max(len(v) for v in by_sym.values())
    tlen = np.zeros((ndup, 512), np.int64)
    tcode = np.zeros((ndup, 512), np.uint64)
    tleaf = np.zeros((ndup, 512), np.int64)
    have = np.zeros(512, bool)
    for s, v in by_sym.items():
        have[s] = True
        for k in range(ndup):
            tlen[k, s], tcode[k, s], tleaf[k, s] = v[k % len(v)]
    return tlen, tcode, tleaf, have


def leaves_used(tree, tokens):
    """Indices (into leaves(tree)) of the leaves that the tokens' codes end at."""
    t = as_tokens(tokens)
    tlen, _, tleaf, _ = _code_tables(tree, 1)
    return np.unique(tleaf[t[:, 2] % tlen.shape[0], t[:, 0]])


def token_code_lengths(tree, tokens, root_leaf_bits=1):
    """Bits of every token: code and extra bits."""
    t = as_tokens(tokens)
    tlen = _code_tables(tree, root_leaf_bits)[0]
    return tlen[t[:, 2] % tlen.shape[0], t[:, 0]] + _EXTRA_BITS[t[:, 0]]


def token_bits(tree, tokens, root_leaf_bits=1):
    """The payload bits.  A symbol with several leaves is carried by the leaf that the token's third
    column names (modulo their number); a tree of one leaf is written with root_leaf_bits per code (the
    encoder writes 1, the reference reads 0)."""
    t = as_tokens(tokens)
    tlen, tcode, _, have = _code_tables(tree, root_leaf_bits)
    sym, extra = t[:, 0], t[:, 1]
    assert have[sym].all(), "a token's symbol has no leaf: %s" % sorted(set(sym[~have[sym]].tolist()))
    assert ((extra >= 0) & (extra < (1 << _EXTRA_BITS[sym]))).all(), "extra bits out of range"
    turn = t[:, 2] % tlen.shape[0]
    clen = tlen[turn, sym]
    val = tcode[turn, sym] | (extra.astype(np.uint64) << clen.astype(np.uint64))
    nbits = clen + _EXTRA_BITS[sym]
    total = int(nbits.sum())
    first = np.cumsum(nbits) - nbits
    k = np.arange(total, dtype=np.int64) - np.repeat(first, nbits)
    return ((np.repeat(val, nbits) >> k.astype(np.uint64)) & np.uint64(1)).astype(np.uint8)


# ---- tables and chunks ------------------------------------------------------------------------------

def single_byte_items(table):
    for i in range(1, 128):
        if table[i] >= 256:
            return i - 1
    return 127


def mapping_bytes(table, n1=None):
    """n1 one-byte entries (table[1..n1]), then 127 - n1 two-byte entries; table[0] is not stored."""
    t = np.asarray(table, np.int64)
    assert t.size == 128
    n1 = single_byte_items(t) if n1 is None else n1
    assert 0 <= n1 <= 127 and ((t[1:n1 + 1] >= 0) & (t[1:n1 + 1] <= 255)).all(), "a one-byte entry must be 0..255"
    two = t[n1 + 1:].astype(np.int16).view(np.uint16)
    return np.concatenate(([n1], t[1:n1 + 1], np.stack((two & 255, two >> 8), 1).ravel())).astype(np.uint8)


def qcfg_bytes(shift_luma, shift_chroma, chroma):
    out = []
    for tab in (shift_luma, shift_chroma) if chroma else (shift_luma,):
        s = np.asarray(tab, np.int64)
        assert s.size == 64 and ((s >= 0) & (s <= 15)).all()
        out.append((s[0::2] << 4) | s[1::2])
    return np.concatenate(out).astype(np.uint8)


def _u32(x):
    return np.array([x & 255, (x >> 8) & 255, (x >> 16) & 255, (x >> 24) & 255], np.uint8)


def _chunk(tag, body):
    body = np.frombuffer(bytes(body), np.uint8) if isinstance(body, (bytes, bytearray)) else np.asarray(body, np.uint8)
    assert len(tag) == 4
    return [np.frombuffer(bytes(tag), np.uint8), _u32(body.size), body]


def lres_body(tree, tokens, root_leaf_bits=1):
    """Tree, then one payload without a block header (a fresh scratch buffer: zero pad bits)."""
    return np.concatenate((tree_bytes(tree), np.packbits(token_bits(tree, tokens, root_leaf_bits), bitorder="little")))


def fres_body(tree, row_tokens, root_leaf_bits=1, headers=True):
    """Tree, then per block row a 15-bit size (two bytes; four with the continuation flag) and the payload.
    The reference packs every row into ONE scratch buffer that it clears once: the pad bits of a row's
    last byte are whatever an earlier row left there.  headers=False: the single-row form."""
    parts = [tree_bytes(tree)]
    scratch = np.zeros(0, np.uint8)
    for tokens in row_tokens:
        bits = token_bits(tree, tokens, root_leaf_bits)
        nbytes = (bits.size + 7) // 8
        if scratch.size < 8 * nbytes:
            scratch = np.concatenate((scratch, np.zeros(8 * nbytes - scratch.size, np.uint8)))
        scratch[:bits.size] = bits
        payload = np.packbits(scratch[:8 * nbytes], bitorder="little")
        if headers:
            if nbytes <= 0x7fff:
                parts.append(np.array([nbytes & 255, nbytes >> 8], np.uint8))
            else:
                lo, hi = (nbytes & 0x7fff) | 0x8000, nbytes >> 15
                parts.append(np.array([lo & 255, lo >> 8, hi & 255, hi >> 8], np.uint8))
        parts.append(payload)
    return np.concatenate(parts)


def assemble(W, H, C, ycbcr, lmap, lres_tree, lres_tokens, shift_luma, shift_chroma, fmap, fres_tree,
             fres_row_tokens, extra_chunks=None, frmt_tail=b"", map_n1=(None, None), root_leaf_bits=1,
             check=True):
    """The stream as a uint8 array.
    extra_chunks: {position: (tag, body) or a list of them}; position 0 is in front of FRMT, 1..5 between
    the known chunks, 6 behind FRES.  frmt_tail: bytes behind FRMT's eleven.  map_n1: (LMAP, FMAP) counts
    of one-byte entries (None: as the encoder counts them).  check: the tokens decode to exactly the
    sizes the geometry asks for."""
    rows, cols = (H + 7) // 8, (W + 7) // 8
    chroma = bool(ycbcr) and C >= 3
    if check:
        mr, mc = (rows + 15) // 16, (cols + 15) // 16
        assert tokens_length(lres_tokens) == C * (mr * mc + rows * cols), "LRES tokens: wrong length"
        assert len(fres_row_tokens) == rows, "one token list per block row"
        for t in fres_row_tokens:
            assert tokens_length(t) == cols * 64 * C, "FRES row tokens: wrong length"
    frmt = np.concatenate((np.array([1], np.uint8), _u32(W), _u32(H), np.array([C, 1 if ycbcr else 0], np.uint8),
                           np.frombuffer(bytes(frmt_tail), np.uint8)))
    known = [
        (b"FRMT", frmt),
        (b"LMAP", mapping_bytes(lmap, map_n1[0])),
        (b"LRES", lres_body(lres_tree, lres_tokens, root_leaf_bits)),
        (b"QCFG", qcfg_bytes(shift_luma, shift_chroma, chroma)),
        (b"FMAP", mapping_bytes(fmap, map_n1[1])),
        (b"FRES", fres_body(fres_tree, fres_row_tokens, root_leaf_bits, headers=rows > 1)),
    ]
    extra_chunks = extra_chunks or {}
    parts = []
    for pos in range(7):
        ex = extra_chunks.get(pos, [])
        for tag, body in ([ex] if isinstance(ex, tuple) else ex):
            parts += _chunk(tag, body)
        if pos < 6:
            parts += _chunk(*known[pos])
    body = np.concatenate([np.frombuffer(b"HIMG", np.uint8)] + parts)
    return np.concatenate((np.frombuffer(b"RIFF", np.uint8), _u32(body.size), body))


def from_trace(W, H, C, ycbcr, tr, **kw):
    """The encoder's own stream from the oracle's trace (oracle_lib.oracle_encode(..., trace=True))."""
    rows, cols = tr["rows"], tr["cols"]
    fres = tr["fres_sym"].reshape(rows, cols * 64 * C)
    return assemble(W, H, C, ycbcr, tr["lmap"], tree_from_codes(tr["lres_len"], tr["lres_code"]),
                    encoder_tokens(tr["lres_sym"]), tr["shift_luma"], tr["shift_chroma"], tr["fmap"],
                    tree_from_codes(tr["fres_len"], tr["fres_code"]), [encoder_tokens(r) for r in fres], **kw)
