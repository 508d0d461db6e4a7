"""The tile map of the plan (csrc/swt_tilemap.h) on the CPU: tests/tilemap_check.cpp includes the header, is compiled with g++ and
run -- once plain and once with -fsanitize=address,undefined (a stand-alone binary; nothing is loaded into Python).

What the program sweeps: n_bytes 0, 1, 127 .. 129, every size's threshold +- 1 and values up to 2^40; slots 1, 2, 3, 7, 6,400 and
10^4; every c SWT_OPT_LANE_TAPER takes (c = 2/8 .. 64/8), with 128 and with 192 bytes as the smallest size; and uniform maps.
What it checks: boundaries rise strictly from 0 and cover [0, n_bytes); tile_of(boundary(t)) == t and tile_of(boundary(t) - 1) ==
t - 1; n_tiles is the count of boundaries the rule gives tile by tile, and every boundary is the rule's; no tile is larger than
384 bytes; a uniform map has tile_count() tiles at t * tile; and plan[] by both forms of the plan kernels (plan_range, plan_search:
the code the kernels run) equals a plain lower bound over the boundaries for random sentence offsets, 300 empty sentences at one
offset and one sentence over all tiles."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "tilemap_check.cpp")
INC = os.path.join(ROOT, "subword-tokenizers_amd", "csrc")


def build_and_run(tmp_path, name, flags):
    cxx = os.environ.get("CXX") or shutil.which("g++")
    if not cxx:
        pytest.fail("no g++: the tile map check is a C++ program")
    exe = str(tmp_path / name)
    r = subprocess.run([cxx, "-std=c++17", "-O1", "-Wall", "-Werror", "-I", INC, SRC, "-o", exe] + flags,
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout[-4000:]
    assert r.stdout.startswith("ok: "), r.stdout[-4000:]


def test_tilemap(tmp_path):
    build_and_run(tmp_path, "tilemap_check", [])


def test_tilemap_sanitized(tmp_path):
    build_and_run(tmp_path, "tilemap_check_san", ["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"])
