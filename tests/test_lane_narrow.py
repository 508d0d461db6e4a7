"""The 16-bit symbol codes of the FastBPE lane kernel (csrc/swt_bpe_narrow.h) on the CPU: tests/narrow_check.cpp includes the
header, is compiled with g++ and run -- once plain and once with -fsanitize=address,undefined (a stand-alone binary; nothing is
loaded into Python).

What the program checks: the alphabet is the ascending set of base code points that are the left or the right of a merge, and
code_of_cp / cp_of_code agree with it; a table is eligible up to letters + merges = 0x7FFD and not one beyond (chain merges over
2, 3 and 45 letters), not when it is not packed, and not when it names a symbol whose code would not fit; the two-choice table of
the codes finds every merge of the pretrained merges.json under rank << 16 | code of the merged symbol (the last of a pair listed
twice), holds nothing else, and misses 10,000 seeded absent pairs."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "narrow_check.cpp")
INC = os.path.join(ROOT, "subword-tokenizers_amd", "csrc")
MERGES = os.path.join(ROOT, "tests", "golden", "ref", "resources", "pretrained", "FastBPE", "merges.json")


def build_and_run(tmp_path, name, flags):
    cxx = os.environ.get("CXX") or shutil.which("g++")
    if not cxx:
        pytest.fail("no g++: the narrow-code check is a C++ program")
    exe = str(tmp_path / name)
    r = subprocess.run([cxx, "-std=c++17", "-O1", "-Wall", "-Werror", "-I", INC, SRC, "-o", exe] + flags,
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout
    r = subprocess.run([exe, MERGES], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout[-4000:]
    assert r.stdout.startswith("ok: 19876 merges of the file over 45 letters"), r.stdout[-4000:]


def test_narrow_codes(tmp_path):
    build_and_run(tmp_path, "narrow_check", [])


def test_narrow_codes_sanitized(tmp_path):
    build_and_run(tmp_path, "narrow_check_san", ["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"])
