"""The normalizer without a device: the plain-Python rule of tests/normalizer_cases.py against the `tokenizers` wheel's recorded
output (tests/golden/bert_normalizer.json), and the argument checks of set_normalizer."""
import pytest

from tests import normalizer_cases as M


def test_model_gives_the_wheels_strings_and_offsets(golden):
    """the normalised strings are the wheel's, and every recorded token's offsets are the model's alignment of the span the token
    takes in the normalised text -- found by walking that text, as the pre-tokenizer does"""
    g = golden("bert_normalizer.json")
    for name, rec in g["settings"].items():
        for text, normalized, tokens, offsets in zip(rec["texts"], rec["normalized"], rec["tokens"], rec["offsets"]):
            got, align = M.normalize(text, rec["flags"])
            assert got == normalized, (name, text)
            at = 0
            for token, (a, b) in zip(tokens, offsets):
                if token in ("[UNK]", "['UNK']"):  # it stands for a whole word: from the next character that is no space to the
                    first = next(k for k in range(at, len(got)) if not got[k].isspace())  # first that comes from behind the span
                    at = next((k for k in range(first, len(align)) if align[k] >= b), len(align))
                    assert (align[first], align[at - 1] + 1) == (a, b), (name, text, token)
                    continue
                piece = token[2:] if token.startswith("##") else token
                at = got.index(piece, at)
                assert M.map_span(at, at + len(piece), align, len(text)) == (a, b), (name, text, token)
                at += len(piece)


def test_set_normalizer_arguments(swt):
    tok = swt.FastWP()
    assert tok.normalizer() is None
    tok.set_normalizer("bert")
    assert tok.normalizer() == M.ALL
    tok.set_normalizer({"lowercase": False})  # strip_accents=None follows lowercase
    assert tok.normalizer() == dict(M.ALL, lowercase=False, strip_accents=False)
    tok.set_normalizer({"strip_accents": True, "lowercase": False, "clean_text": False})
    assert tok.normalizer() == {"clean_text": False, "handle_chinese_chars": True, "strip_accents": True, "lowercase": False}
    for bad, error in (("BERT", TypeError), (["bert"], TypeError), ({"lower": True}, ValueError), ({"lowercase": 1}, TypeError),
                       ({"clean_text": None}, TypeError)):
        with pytest.raises(error):
            tok.set_normalizer(bad)
    assert tok.normalizer()["lowercase"] is False  # a refused argument changes nothing
    tok.set_normalizer(None)
    assert tok.normalizer() is None
    with pytest.raises(ValueError):
        tok.normalize_batch(["a"])
    assert swt.NaiveBPE().normalizer() is None  # the default of every class: encode_batch as it was, no "offset_unit" in its result

