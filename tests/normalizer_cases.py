"""The normalizer's rule (include/swt.h, "The normalizer") as plain Python over unicodedata, and the case lists of its tests.

normalize(text, flags) -> (normalised text, alignment): alignment[k] is the index in `text` of the code point that output
code point k came from.  Evaluated under the interpreter at hand: it speaks for the device's tables only where
unicodedata.unidata_version is theirs (swt_unidata_version)."""
import unicodedata

ALL = {"clean_text": True, "handle_chinese_chars": True, "strip_accents": True, "lowercase": True}
NO_STRIP = dict(ALL, strip_accents=False)
NO_LOWER = dict(ALL, lowercase=False)
ONLY_LOWER = {"clean_text": False, "handle_chinese_chars": False, "strip_accents": False, "lowercase": True}
FLAG_SETS = {"all": ALL, "no_strip": NO_STRIP, "no_lower": NO_LOWER, "only_lower": ONLY_LOWER}
CJK = ((0x4E00, 0x9FFF), (0x3400, 0x4DBF), (0x20000, 0x2A6DF), (0x2A700, 0x2B73F), (0x2B740, 0x2B81F), (0x2B820, 0x2CEAF),
       (0xF900, 0xFAFF), (0x2F800, 0x2FA1F))


def expand(c, flags):
    """what one code point of the text becomes"""
    cat = unicodedata.category(c)
    if flags["clean_text"]:
        if c in "\0\ufffd" or (cat[0] == "C" and c not in "\t\n\r"):
            return ""
        if c in "\t\n\r" or cat in ("Zs", "Zl", "Zp"):
            c = " "
    wrap = " " if flags["handle_chinese_chars"] and any(a <= ord(c) <= b for a, b in CJK) else ""
    out = c
    if flags["strip_accents"]:
        out = "".join(d for d in unicodedata.normalize("NFD", c) if unicodedata.category(d) != "Mn")
    if flags["lowercase"]:
        out = "".join("σ" if d == "Σ" else d.lower() for d in out)
    return wrap + out + wrap


def normalize(text, flags):
    out, align = [], []
    for i, c in enumerate(text):
        e = expand(c, flags)
        out.append(e)
        align.extend([i] * len(e))
    return "".join(out), align


def map_span(a, b, align, n_source):
    """a span [a, b) over the normalised text -> over the original (swt_normalize_spans)"""
    a2 = align[a] if a < len(align) else n_source
    return (a2, align[b - 1] + 1) if b > a else (a2, a2)


# code points assigned long before Unicode 13, so that the wheel's tables and this interpreter's agree on them
TEXTS = ["Zażółć gęślą jaźń", "Pchnąć w tę łódź jeża lub ośm skrzyń fig.", "Élan vital; naïve café, ÀÉÎÕÜ ñ Ç", "tab\there\nnew\r\nline",
         "zero\u200bwidth \u00adsoft\u0000nul \ufffd", "nbsp\u00a0and\u2003em\u2028sep", "中文字符 mixed 漢字text", "한국어 조선말",
         "İstanbul ΙΣΤΟΡΊΑ DŽ ǅ ß ẞ", "e\u0301 combining a\u0308\u0323", "𝐀 math 😀 emoji", "", "   ", "\u200b\u200b", "Ångström Kelvin K Ω",
         "日本語のテキスト", "[MASK] żółw [SEP]", "ǆ ǈ Ǆ", "ᾂ ᾳ ΐ", "ﬁ ligature ½"]

# the probes of the seam test: what they become under ALL is in the comment
PROBES = ["İ",       # 2 bytes -> 'i' (3 with its mark when accents stay)
          "한",      # 3 bytes -> 9: three jamo
          "中",      # 3 bytes -> 5: spaces around it
          "é",       # 2 bytes -> 1
          "\u200b",  # dropped
          "𝐀"]       # 4 bytes, kept
