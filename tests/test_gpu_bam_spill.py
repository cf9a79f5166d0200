"""sam2bam's out-of-core mode (mkt_bam_spill / mkt_bam_pull / mkt_bam_stats, bin/sam2bam -m / -T): the text is cut into runs of a
budget, each run sorted on the GPU and spilled to temporary files, the runs merged on the GPU window by window.  The result must be
the single-pass BAM and BAI byte for byte, whatever the budget; temporary files never stay behind."""
import functools
import os
import subprocess

import pytest

import bamio
import util
from test_gpu_bam import check_bam, header_for

pytestmark = pytest.mark.gpu


@functools.lru_cache(maxsize=None)
def _input(profile, seed, groups):
    body = util.synth(profile, seed, groups)
    hdr, order = header_for(body)
    return hdr, body, order


def _leftovers(prefix):
    d, base = os.path.split(str(prefix))
    return [f for f in os.listdir(d) if f.startswith(base)]


@pytest.mark.parametrize("profile", ["unc", "flash"])
def test_identity_with_any_number_of_runs(profile, tmp_path):
    import microcket_amd as m
    hdr, body, order = _input(profile, 23, 40000)
    for level in (0, 1, 2):
        ref = m.sam_to_bam(hdr + body, sorted=True, level=level)
        # budget above the input: the single pass; equal to the input: ONE spilled run through the merge; then ~8 and >= 100 runs
        for budget, nruns_wanted, spilled in ((len(body) + 1, 1, False), (len(body), 1, True), (len(body) // 8, 8, True), (len(body) // 120, 120, True)):
            st = {}
            got = m.sam_to_bam(hdr + body, sorted=True, level=level, piece=(1 << 22) + 7, run_bytes=budget, tmp=tmp_path / "p", stats=st)
            assert got[2] == ref[2]
            assert got[0] == ref[0], (profile, level, budget)
            assert got[1] == ref[1], (profile, level, budget)
            assert st["runs"] >= nruns_wanted and st["runs"] <= 2 * nruns_wanted + 1, st
            assert (st["tmp_bytes"] > 0) == spilled
            assert _leftovers(tmp_path / "p") == []
        if level == 2:
            check_bam(hdr, body, got[0], got[1], got[2], True, order)


def test_ties_and_unmapped_across_runs(tmp_path):
    """20 000 records at one (reference, position, strand) and unmapped ones spread over >= 20 runs: input order survives the merge"""
    import microcket_amd as m
    lines = []
    for i in range(20000):
        if i % 7 == 3:
            lines.append(f"u{i:05d}\t4\t*\t0\t0\t*\t*\t0\t0\tACGT\tIIII")
        else:
            lines.append(f"t{i:05d}\t16\tchr5\t1000\t60\t4M\t*\t0\t0\tACGT\tIIII")
        if i % 500 == 0:
            lines.append(f"e{i:05d}\t0\tchr1\t{5 + i}\t60\t4M\t*\t0\t0\tACGT\tIIII")
    body = ("\n".join(lines) + "\n").encode()
    hdr, order = header_for(body)
    ref = m.sam_to_bam(hdr + body)
    st = {}
    got = m.sam_to_bam(hdr + body, run_bytes=len(body) // 25, tmp=tmp_path / "t", stats=st, piece=100000)
    assert st["runs"] >= 20
    assert got == ref
    bam = check_bam(hdr, body, got[0], got[1], got[2], True, order)
    names = [r["qname"] for _, _, r in bam.records]
    assert [q for q in names if q[0] == "t"] == [ln.split("\t")[0] for ln in lines if ln[0] == "t"]
    assert [q for q in names if q[0] == "u"] == [ln.split("\t")[0] for ln in lines if ln[0] == "u"]
    assert all(q[0] == "u" for q in names[-sum(1 for ln in lines if ln[0] == "u"):])
    assert bamio.Bai(got[1]).n_no_coor == sum(1 for ln in lines if ln[0] == "u")


def test_edges(tmp_path):
    import microcket_amd as m
    hdr = b"@SQ\tSN:chr1\tLN:1000000\n"
    pre = tmp_path / "e"
    for sam in (hdr, b""):                                            # header only, empty
        assert m.sam_to_bam(sam, run_bytes=100, tmp=pre) == m.sam_to_bam(sam)
    lines = [b"r%05d\t0\tchr1\t%d\t60\t3M\t*\t0\t0\tACG\tIII" % (i, 1 + (i * 7919) % 900000) for i in range(3000)]
    body = b"\n".join(lines) + b"\n"
    ref = m.sam_to_bam(hdr + body)
    st = {}
    assert m.sam_to_bam(hdr + body, run_bytes=len(body) * 2, tmp=pre, stats=st) == ref           # one run, no temporary file
    assert st["runs"] == 1 and st["tmp_bytes"] == 0 and _leftovers(pre) == []
    st = {}
    assert m.sam_to_bam(hdr + body, run_bytes=5, tmp=pre, stats=st, piece=4096) == ref            # a budget below one line
    assert st["runs"] == len(lines) and _leftovers(pre) == []
    crlf = body.replace(b"\n", b"\r\n")                               # \r\n line ends, no final newline
    ref2 = m.sam_to_bam(hdr + crlf[:-2])
    assert ref2[2] == len(lines)
    for budget in (997, 4096, 40000):
        assert m.sam_to_bam(hdr + crlf[:-2], run_bytes=budget, tmp=pre, piece=3001) == ref2
    big = b"@SQ\tSN:chrBig\tLN:600000000\n"                           # beyond the BAI format: the same note, no index
    bl = b"".join(b"b%d\t0\tchrBig\t%d\t0\t1M\t*\t0\t0\tA\tI\n" % (i, 550000000 - i * 1000) for i in range(400))
    n0, n1 = [], []
    r0 = m.sam_to_bam(big + bl, notes=n0)
    r1 = m.sam_to_bam(big + bl, run_bytes=1000, tmp=pre, notes=n1)
    assert r1 == r0 and r1[1] == b"" and n1 == n0 and "no index" in n1[0]
    for level in (0, 2):                                              # input order: pieces as they come, no temporary files
        st = {}
        u = m.sam_to_bam(hdr + body, sorted=False, level=level, run_bytes=20000, piece=7000, tmp=pre, stats=st)
        assert u == m.sam_to_bam(hdr + body, sorted=False, level=level) and st["runs"] >= 4 and st["tmp_bytes"] == 0
    # the data ends exactly on a BGZF block boundary and every record has coordinates: the last chunk of the index ends at the
    # virtual offset of the end of the data, which then is the start of the block after the last one.  Records of this shape take
    # 52 bytes (4 + 32 fixed, 7 name, 4 CIGAR, 2 SEQ, 3 QUAL); an @CO line pads the header.
    lines = [b"r%05d\t0\tchr1\t%d\t60\t3M\t*\t0\t0\tACG\tIII" % (i, 1 + i * 300) for i in range(3000)]
    body = b"\n".join(lines) + b"\n"
    h0, order = header_for(body)
    fixed = 12 + len("@HD\tVN:1.6\tSO:coordinate\n") + len(h0) + sum(9 + len(c) for c in order) + 52 * len(lines)
    pad = -(fixed + 5) % 0xff00
    hdr = h0 + b"@CO\t" + b"x" * pad + b"\n"
    ref = m.sam_to_bam(hdr + body)
    bam = check_bam(hdr, body, ref[0], ref[1], ref[2], True, order)
    assert bam.raw_len == fixed + 5 + pad and bam.raw_len % 0xff00 == 0
    assert bamio.Bai(ref[1]).n_no_coor == 0
    st = {}
    assert m.sam_to_bam(hdr + body, run_bytes=len(body) // 3 + 200, tmp=pre, stats=st, piece=4096) == ref
    assert st["runs"] == 3 and _leftovers(pre) == []


@pytest.mark.parametrize("groups,limit_mb,case", [(64000, 48, "the text does not fit"), (16000, 48, "the text fits, the single pass does not")])
def test_auto_switches_to_runs_where_the_single_pass_would_not_fit(tmp_path, monkeypatch, groups, limit_mb, case):
    """MKT_BAM_DEVICE_LIMIT: the device bytes the object may hold, as if HBM ended there"""
    import microcket_amd as m
    hdr, body, _ = _input("unc", 5, groups)
    ref = m.sam_to_bam(hdr + body)
    st = {}
    assert m.sam_to_bam(hdr + body, run_bytes="auto", tmp=tmp_path / "a", stats=st) == ref and st["runs"] == 1 and st["tmp_bytes"] == 0
    monkeypatch.setenv("MKT_BAM_DEVICE_LIMIT", str(limit_mb << 20))
    with pytest.raises(m.MktError):                                   # without runs the input does not fit
        m.sam_to_bam(hdr + body, piece=1 << 20)
    st = {}
    assert m.sam_to_bam(hdr + body, run_bytes="auto", tmp=tmp_path / "a", stats=st, piece=1 << 20) == ref, case
    assert st["runs"] >= 2 and st["tmp_bytes"] > 0 and st["peak_device_bytes"] <= limit_mb << 20, (case, st)
    assert _leftovers(tmp_path / "a") == []
    if case.startswith("the text fits"):                             # (checked: the whole text was resident before the switch)
        assert len(body) < (limit_mb << 20) // 2


def test_malformed_line_in_a_later_run(tmp_path):
    import microcket_amd as m
    hdr = b"@SQ\tSN:chr1\tLN:1000000\n"
    ok = [b"r%05d\t0\tchr1\t%d\t60\t3M\t*\t0\t0\tACG\tIII" % (i, 1 + i) for i in range(3000)]
    body = b"\n".join(ok[:1350] + [b"r\t0\tchr1\t1\t0\t1Q\t*\t0\t0\tA\tI"] + ok[1350:]) + b"\n"      # (in the third of five runs)
    with pytest.raises(m.MktError) as e0:
        m.sam_to_bam(hdr + body)
    with pytest.raises(m.MktError) as e1:
        m.sam_to_bam(hdr + body, run_bytes=len(body) // 5, tmp=tmp_path / "x", piece=5000)
    assert "not SAM alignment text (error bits 0x8" in str(e1.value)
    assert str(e0.value).split(": ", 2)[2] == str(e1.value).split(": ", 2)[2]
    assert _leftovers(tmp_path / "x") == []


def test_device_memory_is_bounded_by_the_budget(tmp_path):
    import microcket_amd as m
    budget = 1 << 20
    peaks, sizes = [], []
    for groups in (16000, 64000):                                     # 15 MB and 60 MB of text
        hdr, body, _ = _input("unc", 5, groups)
        st = {}
        m.sam_to_bam(hdr + body, run_bytes=budget, tmp=tmp_path / "b", stats=st, piece=1 << 20)
        assert st["runs"] >= len(body) / budget
        peaks.append(st["peak_device_bytes"])
        sizes.append(len(body))
    assert abs(peaks[1] - peaks[0]) <= 0.1 * peaks[0], peaks
    assert peaks[1] < sizes[1] / 2, (peaks, sizes)                    # (the text buffer follows the budget, not the input)


def test_executable_with_runs(tmp_path):
    import microcket_amd.build as b
    exe = b.SAM2BAM
    a = util.synth("flash", 5, 6000)
    c = util.synth("unc", 6, 7000)
    hdr, order = header_for(a + c)
    for name, data in (("h.sam", hdr), ("a.sam", a), ("c.sam", c)):
        (tmp_path / name).write_bytes(data)
    ins = [str(tmp_path / f) for f in ("h.sam", "a.sam", "c.sam")]
    d = tmp_path / "tmp"
    d.mkdir()
    r = subprocess.run([exe, "-o", str(tmp_path / "x.bam")] + ins, capture_output=True)
    assert r.returncode == 0, r.stderr
    want, want_bai = (tmp_path / "x.bam").read_bytes(), (tmp_path / "x.bam.bai").read_bytes()
    r = subprocess.run([exe, "-m", "1M", "-T", str(d / "p"), "-o", str(tmp_path / "y.bam")] + ins, capture_output=True, env=dict(os.environ, MKT_VERBOSE="1"))
    assert r.returncode == 0, r.stderr
    assert (tmp_path / "y.bam").read_bytes() == want and (tmp_path / "y.bam.bai").read_bytes() == want_bai
    assert b"runs formed" in r.stderr and os.listdir(d) == []
    half = (len(hdr) + len(a) + len(c)) // 2 + 1000                  # two runs
    r = subprocess.run([exe, "-m", str(half), "-T", str(d / "p"), "-o", str(tmp_path / "y2.bam")] + ins, capture_output=True, env=dict(os.environ, MKT_VERBOSE="1"))
    assert r.returncode == 0 and b"2 runs formed" in r.stderr, r.stderr
    assert (tmp_path / "y2.bam").read_bytes() == want and (tmp_path / "y2.bam.bai").read_bytes() == want_bai
    # files that merely carry the temporary prefix, but were not made by this run, stay
    (tmp_path / "x.bam.tmp.runs").write_bytes(b"someone else's")
    r = subprocess.run([exe, "-o", str(tmp_path / "x.bam")] + ins, capture_output=True)
    assert r.returncode == 0 and (tmp_path / "x.bam.tmp.runs").read_bytes() == b"someone else's"
    r = subprocess.run([exe, "-m", "1M", "-T", str(d / "p"), "-o", "-", "-"], input=hdr + a + c, capture_output=True)
    assert r.returncode == 0 and r.stdout == want and os.listdir(d) == []
    tgt = tmp_path / "app.bin"
    tgt.write_bytes(b"PREFIX--")
    with open(tgt, "ab") as fo:
        rr = subprocess.run([exe, "-m", "1M", "-T", str(d / "p"), "-o", "-"] + ins, stdout=fo, stderr=subprocess.PIPE)
    assert rr.returncode == 0, rr.stderr
    assert tgt.read_bytes() == b"PREFIX--" + want and os.listdir(d) == []
    r = subprocess.run([exe, "-u", "-m", "1M", "-o", "-"] + ins, capture_output=True)
    r0 = subprocess.run([exe, "-u", "-o", "-"] + ins, capture_output=True)
    assert r.returncode == 0 and r0.returncode == 0 and r.stdout == r0.stdout
    for bad in ("0", "x", "12Q", "-5", "1.5G"):
        assert subprocess.run([exe, "-m", bad, "-o", str(tmp_path / "z.bam")] + ins, capture_output=True).returncode == 2, bad
    r = subprocess.run([exe, "-m", "1M", "-T", str(tmp_path / "nodir" / "p"), "-o", str(tmp_path / "z.bam")] + ins, capture_output=True)
    assert r.returncode == 22 and str(tmp_path / "nodir" / "p").encode() in r.stderr, r.stderr
    bad = tmp_path / "bad.sam"
    bad.write_bytes(c[:len(c) // 2] + b"r\t0\tchr1\t1\t0\t1Q\t*\t0\t0\tA\tI\n" + c[len(c) // 2:])
    r = subprocess.run([exe, "-m", "256K", "-T", str(d / "p"), "-o", str(tmp_path / "z.bam"), ins[0], ins[1], str(bad)], capture_output=True)
    assert r.returncode == 23 and b"not SAM" in r.stderr and os.listdir(d) == []
