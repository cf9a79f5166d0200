"""The lean kernel's piecewise .pairs emitter (fast_emit_part, microcket_amd/csrc/mkt_fast.h) without a GPU: tests/host/emit_parts.cpp,
a stand-alone program, writes hand-made lines piece by piece for parts in {1, 2, 3, 4, 8} between sentinel bytes, pieces and lines
in both orders, and compares every byte with fast_pair_byte.  The program itself checks that its lines reach every destination
alignment with every length mod 4, the 14-byte line, each run boundary on and beside a piece boundary, 10-digit positions and the
longest QNAMEs, and fails when one of them is missing.  Run plain and built with the address and undefined-behaviour sanitizers."""
import subprocess

import pytest

from microcket_amd import build


@pytest.mark.parametrize("which", [0, 1], ids=["plain", "sanitized"])
def test_every_piece_of_every_line(which):
    exe = build.build_emit_parts()[which]
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=120)
    assert r.returncode == 0, (r.returncode, r.stdout.decode(), r.stderr.decode()[-2000:])
    assert r.stdout.startswith(b"emit_parts ok lines "), r.stdout
    assert r.stderr == b"", r.stderr.decode()[-2000:]
