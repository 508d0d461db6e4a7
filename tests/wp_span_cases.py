"""The project's own Python model of the FastWP walk WITH POSITIONS (include/swt.h, swt_wp_encode_spans): what
swt_wp_encode_spans must return, written from SURVEY.md Appendix A.4 / A.5 and independent of csrc/swt_wp.hip.

  the trie      insert, then the breadth-first pass from [root, root_sharp]: an end node fails to root_sharp and pops its own
                token; any other node follows its parent's failure chain, collecting pops, to the first node with an edge for its
                character (none: no link, no pops); a node whose character is not alphanumeric then fails to root_p whatever it had,
                and KEEPS its pops (A.4): the path of the old link target is lost, which is the short cover
  a segment     the walk from i0 over s = text + " " until a node without a link has no edge (i1); valid when i1 is a boundary
                and the node is root, root_sharp or root_p; then on to the next boundary and over white space (A.5)
  the spans     valid: the tokens cover a prefix of s[i0:i1] one after the other, the first len(token) code points, a later one
                len(token) - 2; invalid: "['UNK']" covers (i0, b), b the first boundary at or after i1; the '##' corner: one id
                (the marker len(vocab) + 2 when NaiveWP.encode_word("##") has several tokens) over (i0, i0 + 2)
  the word ids  the segments of a sentence that emit a token, numbered from 0
  statuses      WP_INDEXERROR when the walk reads the appended space away (A.5: iswdbndry indexes s[len(s)]), WP_NONTERMINATING
                when a segment ends where it began or reaches a corner the reference never returns from; no tokens then

Positions are code points of the lowercased text; byte positions follow from the UTF-8 length of every code point (valid UTF-8
only: a str)."""
import numpy as np

WP_OK, WP_NONTERMINATING, WP_INDEXERROR = 0, 1, 2
UNK = "['UNK']"


class _Node:
    __slots__ = ("char", "children", "is_end", "link", "pops", "seen")

    def __init__(self, char, seen):
        self.char, self.seen, self.children, self.is_end, self.link, self.pops = char, seen, {}, False, None, []


def is_punc(c):
    return not c.isalnum() and not c.isspace()


class WpSpanModel:
    def __init__(self, vocab):
        self.tokens = sorted(set(vocab))
        self.index = {t: i for i, t in enumerate(self.tokens)}
        self.n = len(self.tokens)
        self.root, self.root_p = _Node("", ""), _Node("", "")
        self.root_sharp = self._insert("##")
        for t in self.tokens:
            self._insert(t)
        self._links()
        self.corner = self._corner()  # token strings, or None: the reference never returns

    def _insert(self, word):
        node = self.root
        for ch in word:
            nxt = node.children.get(ch)
            if nxt is None:
                nxt = node.children[ch] = _Node(ch, node.seen + ch)
            node = nxt
        node.is_end = True
        return node

    def _links(self):
        queue, head = [self.root, self.root_sharp], 0
        while head < len(queue):
            cur = queue[head]
            head += 1
            for ch, child in cur.children.items():
                if child is self.root_sharp:
                    continue
                if child.is_end:
                    child.link, child.pops = self.root_sharp, [child.seen]
                else:
                    f, acc = cur.link, []
                    while f is not None and ch not in f.children:
                        acc += f.pops
                        f = f.link
                    if f is not None:
                        child.link, child.pops = f.children[ch], cur.pops + acc
                if not child.char.isalnum():
                    child.link = self.root_p
                queue.append(child)

    def _corner(self):
        """NaiveWP.encode_word("##"): longest prefix in the vocabulary, '##' in front of every remainder; the state is the
        number of '#' left, so a state seen twice never ends"""
        vocab, word, out, seen = self.index, "##", [], set()
        while word:
            if word in seen:
                return None
            seen.add(word)
            i = len(word)
            while i > 0 and word[:i] not in vocab:
                i -= 1
            if i == 0:
                return ["[UNK]"]
            out.append(word[:i])
            word = word[i:]
            if word:
                word = "##" + word
            if len(word) > 64:
                return None
        return out

    # ------------------------------------------------------------------------------------------------------------------
    def names(self):
        return self.tokens + [UNK, "[UNK]"]

    def corner_id(self):
        if self.corner is None:
            return None
        if len(self.corner) == 1:
            return self.n + 1 if self.corner[0] == "[UNK]" else self.index[self.corner[0]]
        return self.n + 2

    def sentence(self, text):
        """text (lowercased) -> (ids, spans in code points [(start, end)], word ids, status)"""
        s = text + " "
        n = len(s)
        cls = [(c.isspace(), is_punc(c)) for c in s]

        def bndry(i):
            return (i > 0 and cls[i - 1][1]) or cls[i][0] or cls[i][1]

        ids, spans, word, nw, i = [], [], [], 0, 0
        while i < n:
            i0, node, toks = i, self.root, []
            while i < n:
                stop = False
                while s[i] not in node.children:
                    if node.link is None:
                        stop = True
                        break
                    toks += node.pops
                    node = node.link
                if stop:
                    break
                node = node.children[s[i]]
                i += 1
            if i >= n:
                return [], [], [], WP_INDEXERROR
            i1 = i
            if not bndry(i1) or not (node is self.root or node is self.root_sharp or node is self.root_p):
                b = i1
                while not bndry(b):
                    b += 1
                ids.append(self.n)
                spans.append((i0, b))
                word.append(nw)
                nw += 1
            elif node is self.root_sharp and not toks:
                if self.corner is None:
                    return [], [], [], WP_NONTERMINATING
                ids.append(self.corner_id())
                spans.append((i0, min(i0 + 2, n - 1)))
                word.append(nw)
                nw += 1
            else:
                p = i0
                for k, t in enumerate(toks):
                    L = min(len(t) - 2 if k and t.startswith("##") else len(t), n - 1 - p)  # a span never passes the sentence's end
                    ids.append(self.index[t])
                    spans.append((p, p + L))
                    word.append(nw)
                    p += L
                nw += 1 if toks else 0
            while i < n and not bndry(i):
                i += 1
            while i < n and cls[i][0]:
                i += 1
            if i == i0:
                return [], [], [], WP_NONTERMINATING
        return ids, spans, word, WP_OK

    def batch(self, texts):
        """lowercased texts -> ids uint32[n], offsets uint64[len + 1], status uint8[len], spans in code points uint32[n, 2], spans in
        bytes uint32[n, 2], word uint32[n]"""
        ids, off, st, cp, by, wd = [], [0], [], [], [], []
        for t in texts:
            i, s, w, status = self.sentence(t)
            pre = [0]
            for c in t:
                pre.append(pre[-1] + len(c.encode("utf-8")))
            ids += i
            cp += s
            by += [(pre[a], pre[b]) for a, b in s]
            wd += w
            st.append(status)
            off.append(len(ids))
        return (np.array(ids, dtype=np.uint32), np.array(off, dtype=np.uint64), np.array(st, dtype=np.uint8),
                np.array(cp, dtype=np.uint32).reshape(-1, 2), np.array(by, dtype=np.uint32).reshape(-1, 2), np.array(wd, dtype=np.uint32))

    def rows(self, ids, spans, word):
        """the device's ids, spans and word ids of one sentence in the shape of a fixture row: a multi-token corner spelled out,
        every token of it with the corner's span"""
        names, toks, sp, wd = self.names(), [], [], []
        for t, (a, b), w in zip(map(int, ids), spans, word):
            for name in (self.corner if t == self.n + 2 else [names[t]]):
                toks.append(name)
                sp += [int(a), int(b)]
                wd.append(int(w))
        return toks, sp, wd

    def expand_corner(self, ids):
        """the device's ids -> the reference's token strings (a multi-token corner spelled out)"""
        names, out = self.names(), []
        for t in map(int, ids):
            out += self.corner if t == self.n + 2 else [names[t]]
        return out


# ------------------------------------------------------------------------------------------------- the seam constructions
# Built with the generators of tests/test_gpu_wp_seams.py (the handmade vocabulary with SPANNING, fill, sent, layout) and placed
# from the sizes swt_wp_encode_spans_capacity reports (the no-GPU test passes that file's constants, which
# test_constants_are_the_kernels ties to the source).  Smallest shapes that reach each form; about 0.4 MB of text in all.

def seam_batches(chunk, tile, direct_bytes, direct_sents):
    """[(name, sentences)] over the handmade vocabulary"""
    import random

    from tests.test_gpu_lane_spans import fill, nbytes
    from tests.test_gpu_wp_seams import handmade_words, layout, sent

    W = handmade_words()
    rng = random.Random(4080)
    out = []
    # byte straddles: a 2- and a 4-byte character, a punctuation character and a straddler the speculation cannot certify, across
    # a 64-byte block of tile 1 (staged from (700 + pad) & ~15: off0 = (12 + pad) & 15), across the tile boundary inside a
    # sentence, and across the end of the bytes tile 2 stages (from (1100 + pad) & ~15; the chunk is cut at 1500 + pad)
    straddlers = ["ż", "\U0001F600", ".", "a.b"]
    for pad in range(20):
        starts = [0] + [b + pad for b in (200, 700, 1100, 1500, 2300, 2340, 2400, 2480)]
        end = 2600 + pad
        seams = {"block": ((700 + pad) & ~15) + 64, "tile": tile, "chunk end": ((1100 + pad) & ~15) + chunk}
        for k, (name, seam) in enumerate(seams.items()):
            for j in range(2):
                s = straddlers[(pad + k + 2 * j) % 4]
                p = seam - (nbytes(s) + 1) // 2
                out.append(("straddle %r at %d, seam %s %d, pad %d" % (s, p, name, seam, pad),
                            layout(W, rng, starts, end, [(p, s)], dotted=0 if seam > starts[1] else 1, clean=len(starts) - 1)))
    # a sentence longer than the staged bytes, by one lane in global memory: single-launch and tiled
    base = W.plain + W.soft + W.span
    for n in (chunk + 76, chunk + 476, 2 * chunk + 52):
        out.append(("giant of %d bytes" % n, [sent(W, 40, rng, 0), "", fill(base, n, rng), "", sent(W, 40, rng, 1)]))
    out.append(("giant of %d bytes behind a tile" % (chunk + 76), [sent(W, tile + 30, rng), "", fill(base, chunk + 76, rng), "", sent(W, 30, rng)]))
    # the direct form's limits
    for total in (direct_bytes, direct_bytes + 1):
        batch = [sent(W, 300, rng) for _ in range(5)]
        batch.append(sent(W, total - sum(map(nbytes, batch)), rng, 1))
        out.append(("%d bytes in %d sentences" % (total, len(batch)), batch))
    for n in (direct_sents, direct_sents + 1):
        out.append(("%d sentences" % n, [sent(W, rng.randrange(0, 30), rng) for _ in range(n)]))
    # phases C and D mixed: every other sentence holds what the speculation cannot certify
    out.append(("6 KB, every other sentence uncertified", [sent(W, 60, rng, 1 if i % 2 else 0) for i in range(100)]))
    # runs of empty sentences at the start, in the middle and at the end
    for body in (30, 700):
        out.append(("empty runs around sentences of %d bytes" % body,
                    [""] * 3 + [sent(W, body, rng), sent(W, body, rng, 1)] + [""] * 5 + [sent(W, body, rng), sent(W, body, rng)] + [""] * 4))
    return out
