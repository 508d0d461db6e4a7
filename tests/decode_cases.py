"""The project's own Python model of decoding (include/swt.h, swt_decode_plan / swt_decode_rows) and the builders
of its test cases.  The reference's recover_sentence (utils.py:141-154) joins the tokens with spaces and runs three regular
expressions over the string; vocabulary tokens hold no whitespace, so that is a rule about the join between two consecutive
kept tokens, and the rule is what this file holds.  tests/golden/recover_sentence.json pins it to the reference's own strings."""
import numpy as np

GLUE, NO_SPACE_BEFORE, NO_SPACE_AFTER, SPECIAL, BAD = 1, 2, 4, 8, 16
SKIP_SPECIAL, IDS64 = 1, 4  # the flags of a call
STATUS_ID, STATUS_BAD = 1, 2  # the bits of a row's status
SPECIALS = ("[PAD]", "[UNK]", "[CLS]", "[SEP]")
SKIPPED = ("[PAD]", "[CLS]", "[SEP]", "[MASK]")  # what skip_special_tokens leaves out: [UNK] stands for a word of the text
MASK = "[MASK]"
P = frozenset(".,)]\\’-'/")  # no space before a token that starts with one of these
Q = frozenset("([\\’-'/")  # no space after a token that ends with one of these
# the code points Python's \s matches: a token that holds one is not spelled by the rule
WS = frozenset(list(range(0x09, 0x0E)) + list(range(0x1C, 0x21)) + [0x85, 0xA0, 0x1680] + list(range(0x2000, 0x200B)) +
               [0x2028, 0x2029, 0x202F, 0x205F, 0x3000])
# the alphabet of the fixture's exhaustive part, and the wider one of its fuzz
ALPHABET = ["ab", "##cd", "##", "###", "#", ".", "(", "-", "’", "##.", "##(", "x’", "’x", "é"]
FUZZ_ALPHABET = ALPHABET + ["[PAD]", "[UNK]", "[CLS]", "[SEP]", "[MASK]", "['UNK']", ",", ")", "]", "[", "\\", "'", "/", "##-", "##’", "##'x",
                            "a.", ".a", "(a", "a(", "##é", "é’", "中", "##日", "\U0001F600", "####", "#a", "a##b", "##a##"]


def token_flags(tok, special=False):
    """the flag byte of one token string"""
    f = SPECIAL if special else 0
    if not tok or any(ord(c) in WS for c in tok):
        return f | BAD
    if len(tok) >= 3 and tok.startswith("##"):
        f |= GLUE
    if tok[0] in P:
        f |= NO_SPACE_BEFORE
    if tok[-1] in Q:
        f |= NO_SPACE_AFTER
    return f


def join(tokens):
    """recover_sentence(tokens) by the rule, for tokens that are not BAD"""
    out, prev = [], None
    for tok in tokens:
        f = token_flags(tok)
        assert not f & BAD, tok
        if prev is None:
            out.append(tok)
        elif f & GLUE:
            out.append(tok[2:])
        elif f & NO_SPACE_BEFORE or prev & NO_SPACE_AFTER:
            out.append(tok)
        else:
            out.append(" " + tok)
        prev = f
    return "".join(out)


def tables(tokens, mask_id=None):
    """-> (tok_bytes uint8, tok_off uint32[n + 1], tok_flags uint8[n], n): the vocabulary of a call; "[MASK]" is appended when
    mask_id is one past the end"""
    tokens = list(tokens)
    if mask_id is not None and mask_id == len(tokens):
        tokens.append(MASK)
    raw = [t.encode("utf-8") for t in tokens]
    off = np.zeros(len(raw) + 1, dtype=np.uint32)
    off[1:] = np.cumsum([len(b) for b in raw])
    flags = np.array([token_flags(t, t in SKIPPED) for t in tokens], dtype=np.uint8)
    return np.frombuffer(b"".join(raw) + b"\0", dtype=np.uint8)[:-1].copy(), off, flags, len(tokens)


def decode(ids, mask, tabs, flags=SKIP_SPECIAL):
    """the ABI on an id matrix -> (text uint8, text_off uint64[rows + 1], status uint8[rows], info uint64[3])"""
    tok_bytes, tok_off, tok_flags, n_tok = tabs
    raw = tok_bytes.tobytes()
    rows, width = ids.shape
    text, text_off, status, kept = [], np.zeros(rows + 1, dtype=np.uint64), np.zeros(rows, dtype=np.uint8), 0
    total = 0
    for r in range(rows):
        prev = None
        for c in range(width):
            if mask is not None and not mask[r, c]:
                continue
            i = int(ids[r, c])
            if not 0 <= i < n_tok:
                status[r] |= STATUS_ID
                kept += 1
                continue
            f = int(tok_flags[i])
            if flags & SKIP_SPECIAL and f & SPECIAL:
                continue
            kept += 1
            if f & BAD:
                status[r] |= STATUS_BAD
                continue
            b = raw[int(tok_off[i]):int(tok_off[i + 1])]
            if prev is None:
                piece = b
            elif f & GLUE:
                piece = b[2:]
            elif f & NO_SPACE_BEFORE or prev & NO_SPACE_AFTER:
                piece = b
            else:
                piece = b" " + b
            prev = f
            text.append(piece)
            total += len(piece)
        text_off[r + 1] = total
    info = np.array([total, int(np.count_nonzero(status)), kept], dtype=np.uint64)
    return np.frombuffer(b"".join(text) + b"\0", dtype=np.uint8)[:-1].copy(), text_off, status, info


def strings(text, text_off):
    raw = np.asarray(text, dtype=np.uint8).tobytes()
    return [raw[int(a):int(b)].decode("utf-8") for a, b in zip(text_off[:-1], text_off[1:])]


# ---- the vocabulary and the rows of the GPU tests -------------------------------------------------------------------------
LONG = "długi" * 14  # 84 bytes
TOY = list(SPECIALS) + ["ab", "##cd", ".", "(", "’", "x’", "’x", "é", "##", "###", "##(", LONG, "a\u001db", "-", "##" + LONG]
TOY_BAD = TOY.index("a\u001db")


def toy_ids():
    ix = {t: i for i, t in enumerate(TOY)}
    return ix, len(TOY)  # no "[MASK]" in the list: mask_id is one past the end


def random_rows(rows, width, seed, dtype=np.int32):
    """-> (ids, mask): every token of the toy vocabulary but the BAD one, and mask_id; a fifth of the mask zero, with ids there
    that must not be looked up; every third row padded on the left, the last row without a kept column"""
    rng = np.random.default_rng(seed)
    pool = np.array([i for i in range(len(TOY) + 1) if i != TOY_BAD], dtype=np.int64)
    ids = pool[rng.integers(0, pool.size, size=(rows, width))]
    mask = (rng.random((rows, width)) < 0.8).astype(np.uint8)
    for r in range(0, rows, 3):
        mask[r, :rng.integers(0, width + 1)] = 0
    mask[rows - 1] = 0
    ids[mask == 0] = rng.choice(np.array([-1, -100, len(TOY) + 1, 1 << 20, 0, 4]), size=int((mask == 0).sum()))
    return ids.astype(dtype), mask


def seam_rows(width, cols):
    """-> (ids int64[rows, width], mask uint8[rows, width]): rows of "ab" with one token of each kind (glued, P, Q, the
    three-byte quote) on either side of every quad (= lane) boundary near the seams and of every step boundary, and with a
    stretch of skipped columns (mask zeros, specials, left padding) across the boundary between two kept tokens and before a
    first kept glued token"""
    ix, mask_id = toy_ids()
    kinds = [ix["##cd"], ix["."], ix["("], ix["’"], ix["##("], ix[LONG]]
    bounds = sorted({b for b in (4, 8, 60, 64, cols - 4, cols, cols + 4, 2 * cols) if 0 < b < width})
    rows, masks = [], []

    def add(row, mask=None):
        rows.append(row)
        masks.append(np.ones(width, dtype=np.uint8) if mask is None else mask)

    for b in bounds or [0]:
        for k in kinds:
            for d in (-1, 0):
                if 0 <= b + d < width:
                    row = np.full(width, ix["ab"], dtype=np.int64)
                    row[b + d] = k
                    add(row)
            # skipped columns straddle the boundary, a token of the kind right after them
            lo, hi = max(b - 2, 0), min(b + 2, width - 1)
            if hi <= lo:
                continue
            for form in range(3):
                row = np.full(width, ix["ab"], dtype=np.int64)
                mask = np.ones(width, dtype=np.uint8)
                row[hi] = k
                if form == 0:
                    mask[lo:hi] = 0
                    row[lo:hi] = -7  # not looked up
                elif form == 1:
                    row[lo:hi] = [ix["[SEP]"], mask_id, ix["[CLS]"], ix["[PAD]"]][:hi - lo]
                else:  # left padding: nothing kept before the kind
                    row[:hi] = ix["[PAD]"]
                    mask[:hi] = 0
                add(row, mask)
    add(np.full(width, ix["[PAD]"], dtype=np.int64))  # nothing kept
    add(np.full(width, ix["ab"], dtype=np.int64), np.zeros(width, dtype=np.uint8))  # the last row empty
    return np.stack(rows), np.stack(masks)
