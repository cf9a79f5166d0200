"""mkt::ChunkedFile (microcket_amd/csrc/mkt_chunked_file.h), the one writer behind every table bin/pairs2matrix writes in pieces.  The
executables reach its second piece only past 32 MiB of text; tests/host/chunked_file.cpp, a stand-alone program, runs it with a
threshold of 16 bytes: pieces, truncation, the empty file and the failure of a path that cannot be written.  Run plain and built with
the address and undefined-behaviour sanitizers; nothing of it is loaded into python."""
import os
import subprocess

import pytest

import util

HOST = os.path.join(util.ROOT, "tests", "host", "_build", "chunked_file")


@pytest.mark.parametrize("san", [False, True], ids=["plain", "sanitized"])
def test_pieces_truncation_empty_file_and_failure(san, tmp_path):
    util.ensure_built()
    exe = HOST + "_san" if san else HOST
    assert os.path.exists(exe), exe
    r = subprocess.run([exe, str(tmp_path)], stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    assert (r.returncode, r.stdout, r.stderr) == (0, b"ok\n", b"")
    assert sorted(os.listdir(tmp_path)) == ["edge.txt", "emptied.txt", "empty.txt", "many.txt", "one.txt"]
