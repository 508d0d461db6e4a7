"""The project's own model of UnigramWP (include/swt.h, swt_wp_encode_viterbi) in plain Python: float32 totals, one add per candidate."""
import numpy as np

from tests.dropout_cases import words_of


class Model:
    def __init__(self, vocab, scores, max_word_chars=100):
        self.vocab, self.max_word_chars = set(vocab), max_word_chars
        self.ids = {t: k for k, t in enumerate(sorted(self.vocab))}
        self.unk = len(self.ids) + 1
        self.score = {t: np.float32(scores[t]) for t in self.vocab}

    def encode_word(self, word):
        n = len(word)
        if n > self.max_word_chars:
            return ["[UNK]"]
        best, back = [np.float32(0.0)] + [None] * n, [None] * (n + 1)
        for j in range(1, n + 1):
            for i in range(j):
                piece = word[i:j] if i == 0 else "##" + word[i:j]
                if best[i] is None or piece not in self.vocab:
                    continue
                cand = best[i] + self.score[piece]
                if best[j] is None or cand > best[j]:
                    best[j], back[j] = cand, (i, piece)
        if best[n] is None:
            return ["[UNK]"]
        out, j = [], n
        while j:
            j, piece = back[j]
            out.append(piece)
        return out[::-1]

    def tokenize(self, split, texts):
        return [[t for word, _ in words_of(split, text.lower()) for t in self.encode_word(word)] for text in texts]

    def ids_of(self, tokens):
        return [self.unk if t == "[UNK]" else self.ids[t] for t in tokens]

    def batch(self, split, texts):
        """(ids, offsets, status) as the device must give them"""
        rows = [self.ids_of(row) for row in self.tokenize(split, texts)]
        off = np.cumsum([0] + [len(r) for r in rows]).astype(np.uint64)
        return np.array([i for r in rows for i in r], dtype=np.uint32), off, np.zeros(len(texts), dtype=np.uint8)


def dyadic(vocab, seed, span=40):
    """a multiple of 2^-8 below 16 in magnitude per token, from few enough values that totals tie: every float32 sum is exact"""
    rng = np.random.RandomState(seed)
    return {t: float(rng.randint(-span, 1)) / 256.0 * 8 for t in sorted(vocab)}


# MaxMatch says abc ##d ##e, the fewest pieces are ab ##cde; at equal scores "abcd" ties three ways and a ##bcd ends longest
HANDMADE = ["a", "ab", "abc", "##b", "##c", "##d", "##e", "##cd", "##cde", "##bcd", "x", "##x", "ż", "##ół", "##ó", "##ł", "żó", "€", "##€ż",
            "\U0001F600", "##\U0001F600", "##\U0001F600a", "中", "##中ż"]
WORDS = ["a", "ab", "abcd", "abcde", "abx", "xq", "q", "qab", "żół", "żó", "€€ż", "\U0001F600\U0001F600a", "中中ż", "xxxx", "abcdx", ",", "ab-x", "x" * 100,
         "x" * 101, "ab" + "x" * 98, "abc" + "x" * 98]
