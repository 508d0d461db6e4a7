"""The pattern table and the lookup "the longest pattern that matches here" of the added-token search (csrc/swt_added.h) on the
CPU: tests/added_check.cpp includes the header, is compiled with g++ and run -- once plain and once with
-fsanitize=address,undefined (a stand-alone binary; nothing is loaded into Python).

The program builds the table of every case, finds the matches of every text with the shared lookup under the leftmost-longest
rule and blanks them; the matches and the blanked bytes it is held to are those of the model (tests/added_cases.py): the seam
texts, the overlap cases, 4096 patterns sharing a first byte, and the wheel's recorded cases.  It also checks that the edge table
stays at most half full and that build() refuses what include/swt.h says it refuses."""
import os
import shutil
import subprocess

import pytest

from tests import added_cases as A

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "added_check.cpp")
INC = os.path.join(ROOT, "subword-tokenizers_amd", "csrc")
REFUSED = [b"", b"q" * 65, "\U0001F600".encode(), b"\xed\xa0\x80", b"\xc3", b"\x80", b"\xc0\x80", b"\xe0\x80\x80", b"a\xff", b"a\0b"]


def _hex(b):
    return b.hex() if b else "-"


def cases():
    step = 1024
    out = [A.seam_texts(step)] + A.overlap_cases() + [A.many_patterns()] + [(added, texts) for _, added, texts in A.golden_cases(step)]
    return [(list(added), [t.lower() for t in texts]) for added, texts in out]


def write_cases(path):
    n_texts = n_matches = 0
    with open(path, "w", encoding="ascii") as f:
        for added, texts in cases():
            patterns = A.patterns_of(added)
            for p in patterns:
                f.write("P %s\n" % _hex(p.encode("utf-8")))
            f.write("B\n")
            for text in texts:
                matches = A.find_matches(text, patterns)
                rec = []
                for pat, s, e in matches:
                    b0, b1 = A.byte_span(text, s, e)
                    rec += [pat, b0, b1 - b0]
                f.write("T %s %s %d %s\n" % (_hex(text.encode("utf-8")), _hex(A.blank(text, matches).encode("utf-8")), len(matches),
                                             " ".join(map(str, rec))))
                n_texts += 1
                n_matches += len(matches)
        for p in REFUSED:
            f.write("R %s\n" % _hex(p))
    return n_texts, n_matches


def build_and_run(tmp_path, name, flags):
    cxx = os.environ.get("CXX") or shutil.which("g++")
    if not cxx:
        pytest.fail("no g++: the added-token table check is a C++ program")
    exe, data = str(tmp_path / name), str(tmp_path / (name + ".txt"))
    n_texts, n_matches = write_cases(data)
    assert n_texts > 150 and n_matches > 500
    r = subprocess.run([cxx, "-std=c++17", "-O1", "-Wall", "-Werror", "-I", INC, SRC, "-o", exe] + flags,
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout
    r = subprocess.run([exe, data], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout[-4000:]
    assert r.stdout.startswith("ok: %d tables, %d texts, %d matches, %d patterns refused" % (len(cases()), n_texts, n_matches, len(REFUSED))), \
        r.stdout[-4000:]


def test_added_table(tmp_path):
    build_and_run(tmp_path, "added_check", [])


def test_added_table_sanitized(tmp_path):
    build_and_run(tmp_path, "added_check_san", ["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"])
