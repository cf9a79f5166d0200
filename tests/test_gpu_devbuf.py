"""The owning buffer types of microcket_amd/csrc/mkt_devbuf.h (GrowBuf, DevBuf and their pinned counterparts) on a real device,
through the stand-alone program tests/host/devbuf_check.cpp: growth with and without the contents kept, failed allocations that
leave the buffer empty (regrow) or untouched (regrow_keep), moves.  The contexts of the C ABI grow every buffer through them."""
import subprocess

import pytest

import util

pytestmark = pytest.mark.gpu


def test_devbuf_check():
    util.ensure_built()
    r = subprocess.run([util.DEVBUF_CHECK_EXE], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=120)
    out = r.stdout.decode(errors="replace")
    print(out)
    lines = out.splitlines()
    assert r.returncode == 0, out
    assert not [ln for ln in lines if ln.startswith("FAIL")], out
    checks = [ln for ln in lines if ln.startswith("ok  ")]
    assert lines and lines[-1] == "devbuf_check: %d checks passed" % len(checks), out
    # every shape of the check list is there
    for what in ("regrow_keep(2000, 1000): the first 1000 elements are identical", "regrow_keep on an empty buffer with keep = 0 succeeds",
                 "regrow_keep with keep = the old capacity keeps all of it", "an ensure of what fits reallocates nothing",
                 "regrow of a larger size updates the capacity", "after it the buffer is empty with capacity 0",
                 "after it the old pointer, capacity and contents are intact", "self-move-assignment is harmless",
                 "pinned move-assignment transfers, a self-move is harmless", "DevBuf::release hands the pointer over, the owner is empty",
                 "the caller frees what was released (the owner did not)"):
        assert "ok   " + what in lines, what
