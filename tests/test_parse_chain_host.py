"""What the lean kernel's heads phase leaves for its parser and the parser's QNAME compare (fast_head_line, fast_head_ws, lean_eq in
microcket_amd/csrc/mkt_fast.h) without a GPU: tests/host/parse_chain.cpp, a stand-alone program.  The line start and the
short-line verdict against a byte loop for the newline at every byte of its vector, alone and beside a second one, and for the
block's first line; the compare against memcmp for every length 1 .. 101 at every pair of dword offsets with one differing byte
at every position, the bytes behind the ranges always different, one side 11 bytes before the end of its allocation; the separator
words against a bit-by-bit shift for every line start.  Run plain and built with the address and undefined-behaviour sanitizers."""
import subprocess

import pytest

from microcket_amd import build


@pytest.mark.parametrize("which", [0, 1], ids=["plain", "sanitized"])
def test_heads_results_and_qname_compare(which):
    exe = build.build_parse_chain()[which]
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=120)
    assert r.returncode == 0, (r.returncode, r.stdout.decode(), r.stderr.decode()[-2000:])
    assert r.stdout.startswith(b"parse_chain ok row starts "), r.stdout
    assert r.stderr == b"", r.stderr.decode()[-2000:]
