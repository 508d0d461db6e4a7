"""Added and special tokens written in the text (include/swt.h, the added-tokens block) as plain Python over strings and lists:
the match rule, the blanking, the splice and the dense-id rule, and the generators of the seam cases.  No NumPy in the model, no
device, and nothing of the library: tests/test_added_cases.py holds it to the `tokenizers` wheel's recorded output, the GPU tests
hold the library to it."""
import random

MASK = "[MASK]"
BLANKS = {1: " ", 2: "\u00a0", 3: "\u2003"}  # a whitespace code point of every UTF-8 length a pattern may hold


def patterns_of(added):
    """added: [(content, special)] -> the strings that are searched for: content.lower()"""
    return [content.lower() for content, _ in added]


def find_matches(text, patterns):
    """text: one lowercased text -> [(pattern index, start, end)] in code points: among the patterns that match at a position the
    longest wins; from the left, a match is taken at the first position that has one and does not lie inside the match before it;
    the scan goes on at the match's end"""
    out, i = [], 0
    while i < len(text):
        best = -1
        for k, p in enumerate(patterns):
            if text.startswith(p, i) and (best < 0 or len(p) > len(patterns[best])):
                best = k
        if best < 0:
            i += 1
            continue
        out.append((best, i, i + len(patterns[best])))
        i += len(patterns[best])
    return out


def blank(text, matches):
    """the text with every code point of every match replaced by a whitespace code point of its UTF-8 length"""
    chars = list(text)
    for _, s, e in matches:
        for i in range(s, e):
            chars[i] = BLANKS[len(chars[i].encode("utf-8"))]
    return "".join(chars)


def byte_span(text, s, e):
    """code points [s, e) of text as a byte range of its UTF-8"""
    return len(text[:s].encode("utf-8")), len(text[:e].encode("utf-8"))


def splice(tokens, matches, added_base):
    """tokens: [(id, (start, end), word)] of ONE text, encoded from its blanked form; matches: find_matches of it
    -> the same with the matches in their places: a token that starts after j matches has its word index raised by j; a match is
    a word of its own, with the id added_base + pattern"""
    out, t = [], 0
    for k, (pat, s, e) in enumerate(matches):
        while t < len(tokens) and tokens[t][1][0] < s:
            out.append((tokens[t][0], tokens[t][1], tokens[t][2] + k))
            t += 1
        out.append((added_base + pat, (s, e), (tokens[t - 1][2] + 1 if t else 0) + k))
    out.extend((i, sp, w + len(matches)) for i, sp, w in tokens[t:])
    return out


def dense_ids(base_tokens, mask_id, added):
    """The dense-id rule.  base_tokens: the vocabulary's strings in dense-id order (a string listed twice keeps its first index);
    mask_id: the dense id of "[MASK]" over it (its index, or len(base_tokens)).  -> (tokens, dense): the token list with the
    added tokens behind it -- unchanged while nothing is appended, else up to the highest id with "[MASK]" at its reserved slot --
    and the dense id of every added token."""
    index = {}
    for i, t in enumerate(base_tokens):
        index.setdefault(t, i)
    tokens, dense = list(base_tokens), []
    nxt = max(len(base_tokens), mask_id + 1)
    for content, special in added:
        s = content if special else content.lower()
        if s in index:
            dense.append(index[s])
        elif s == MASK:
            dense.append(mask_id)
        else:
            if len(tokens) < nxt:
                tokens.append(MASK)
            index[s] = nxt
            tokens.append(s)
            dense.append(nxt)
            nxt += 1
    return tokens, dense


def refusal(token, n_so_far, is_space):
    """why add_tokens refuses a token, or None.  is_space(ch): the pre-tokenizer drops the code point"""
    if token == "":
        return "empty"
    both = token + token.lower()
    if any(is_space(ch) or ch.isspace() for ch in both):
        return "whitespace"
    if any(ord(ch) > 0xFFFF or ord(ch) == 0 or 0xD800 <= ord(ch) < 0xE000 for ch in both):
        return "code point"
    if len(token.lower().encode("utf-8")) > 64:
        return "long"
    if n_so_far >= 4096:
        return "many"
    return None


# ---- cases

WORDS = ["example", "exam", "exa", "ex", "is", "a", "t", "e", "i", "s", "examples", "test", "exams", "."]


def filler(n_bytes, seed):
    """words of the small WordPiece vocabulary, exactly n_bytes bytes of ASCII, no '[', '<' or '|' inside"""
    rng, out = random.Random(seed), ""
    while len(out) < n_bytes:
        out += rng.choice(WORDS) + " "
    return out[:n_bytes]


def seam_texts(step, added=((MASK, True), ("<user>", True), ("été€", False))):
    """Texts that put matches on the seams of the find kernel's walk (step bytes a step, 64 the longest pattern).
    -> (added, texts)"""
    texts = []
    for k in range(step - 64, step + 2):  # a match starting at every byte around the first step's end
        texts.append(filler(k, k) + "[mask]" + filler(9, k + 1))
    for k in (step - 9, step - 8, step - 1, step):  # a pattern of two- and three-byte code points over the seam, tokens behind it
        texts.append(filler(k, k) + "Été€ examété€ ex")
    texts += ["[MASK]", "[MASK] exam", "exam [MASK]", "[MASK][MASK]", "ex[MASK][mask]am[MASK]", "x<user>x", "", "[mask", "mask]", "",
              "[MASK]", "", "", "<user> [MASK] <user>", "exam <use", "r> exam",  # a would-be match across two texts' boundary
              filler(3 * step + 17, 5) + " [MASK] exam <user>",  # several steps, matches only in the last one
              "[MASK] " * 70 + "exam",  # more than 64 matches in one text
              "[mask]" * 70,  # more than 64 candidates in one step: every '[' is one
              "a été€été€ b été € été€"]
    return list(added), texts


def overlap_cases():
    """[(added, texts)]: ab / abc / bcd over abcd and abcbcd; a prefix of another pattern where the longer one fails at its last
    byte; a 64-byte pattern; a candidate at every byte of a step, every second one a match"""
    long = "<" + "q" * 62 + ">"
    return [([("ab", False), ("abc", False), ("bcd", False)], ["abcd", "abcbcd", "xabcd abcbcdx", "ababcd", "bcdabc"]),
            ([("exam", False), ("example", False)], ["exampl", "example", "exampla example exam", "examexample"]),
            ([("q", False), ("qq", False)], ["q" * 131, "q", "qq", "qqq", "exam" + "q" * 64 + "exam", "qexqqamq"]),
            ([(long, False), ("<q", False)], [long, "a" + long + "b", long[:-1] + "x", long + long, " " + long[:40]])]


def golden_cases(step=1024):
    """[(name, added, texts)]: what tests/golden/make_golden_added_tokens.py records from the `tokenizers` wheel.  Special tokens
    stand in the registered case only (the wheel matches them on the raw text, this library on the lowercased one), no special and
    ordinary pattern overlap, and no text holds U+03A3."""
    added = [(MASK, True), ("<user>", True), ("[SEP]", True), ("été€", False), ("Exams", False)]
    basic = ["[MASK]", "[MASK] exam", "exam [MASK]", "[MASK][MASK]", "ex[MASK][MASK]am[MASK]", "x<user>x", "", "[mask", "MASK]",
             "<user> [MASK] <user>", "exam <use", "r> exam", "Paris is the [MASK] of France.", "a Été€été€ b été € Été€ t",
             "Example[SEP]exams is a test. [SEP]", "EXAMS exam examsexams", "[MASK] " * 70 + "exam", "  [MASK]  .[MASK].  "]
    seams = [filler(k, k) + "[MASK]" + filler(9, k + 1) for k in (step - 64, step - 7, step - 6, step - 5, step - 1, step, step + 1)]
    seams += [filler(k, k) + "Été€ examété€ ex" for k in (step - 9, step - 8, step - 1)]
    seams.append(filler(3 * step + 17, 5) + " [MASK] exam <user>")
    out = [("basic", added, basic), ("seams", added, seams)]
    out += [("overlap%d" % i, a, t) for i, (a, t) in enumerate(overlap_cases())]
    return out


def many_patterns(n=4096):
    """n patterns sharing their first byte, and texts that hold a few of them"""
    added = [("<%04x>" % k, False) for k in range(n)]
    texts = ["exam <0000> <%04x> is" % (n - 1), "<0fff><0ffg> <00", "<0123><0123>", "a<07ff>b"]
    return added, texts
