"""bin/pairs2matrix with every analysis switched on in ONE command line.  The other GPU tests run each analysis's flags on their own;
what they cannot see is one analysis disturbing another when all of them share a run: results in the library invalidate each other, so
the order of the calls matters.  Here the set of files written is exactly the documented one, and every file is byte for byte the file
of a run with only the switches that file needs ("without the flag ... every other byte is the same", from the other side).
MKT_PAIRS2MATRIX names another binary to hold to the same test."""
import os
import subprocess

import numpy as np
import pytest

import microcket_amd as m
import util

pytestmark = pytest.mark.gpu

EXE = os.environ.get("MKT_PAIRS2MATRIX") or os.path.join(util.ROOT, "microcket_amd", "bin", "pairs2matrix")
TABLE = [("chr1", 250300), ("chr2", 120700), ("chrV", 17250)]               # at 5000 and at 1000 every chromosome ends in a partial bin
RES = [5000, 1000]
BALANCE = ["--balance", "--min-nnz", "1", "--mad-max", "0"]

PER_RES = {"base": ["coo", "bins.bed", "weights.bed", "expected.tsv", "expected.chrom.tsv", "expected.trans.tsv"], "apa": ["loops.bedpe", "apa.tsv"], "pileup": ["pileup.tsv"],
           "saddle": ["eigs.tsv", "saddle.tsv"], "insulation": ["insulation.tsv"], "compare": ["scc.tsv"], "viewpoint": [], "hic": []}
ONCE = {"base": ["matrix.stat", "balance.stat"], "apa": ["loops.stat", "apa.stat"], "pileup": ["pileup.stat"], "saddle": ["eigs.stat", "saddle.stat"],
        "insulation": ["insulation.stat"], "compare": ["scc.stat"], "viewpoint": ["viewpoint.bedgraph", "viewpoint.links", "partners.bedgraph", "viewpoint.stat"],
        "hic": ["hic", "hic.stat"]}


def _pairs(n, seed):
    """n pairs: two thirds cis with a decaying distance, the rest anywhere, every tenth one on the viewpoint, a few past a chromosome's end"""
    rng = np.random.default_rng(seed)
    L = np.array([l for _, l in TABLE], dtype=np.int64)
    ia = rng.choice(3, size=n, p=[0.6, 0.3, 0.1])
    ib = np.where(rng.random(n) < 0.67, ia, rng.choice(3, size=n, p=[0.5, 0.3, 0.2]))
    pa = 1 + (rng.random(n) * L[ia]).astype(np.int64)
    near = np.clip(pa + (rng.exponential(8000.0, size=n) * rng.choice([-1, 1], size=n)).astype(np.int64), 1, L[ia])
    pb = np.where(ia == ib, near, 1 + (rng.random(n) * L[ib]).astype(np.int64))
    pb[::97] += 400000                                                      # skipped: past the end
    names = [nm for nm, _ in TABLE]
    return "".join(f"q\t{names[a]}\t{p}\t{names[b]}\t{q}\t+\t-\n" for a, p, b, q in zip(ia.tolist(), pa.tolist(), ib.tolist(), pb.tolist())).encode()


def test_every_switch_at_once_writes_each_file_as_its_own_switches_do(tmp_path):
    if m.device_count() < 1:
        pytest.fail("no HIP device")
    if not os.path.exists(EXE):
        from microcket_amd import build
        build.build_pairs2matrix()
    (tmp_path / "g.sizes").write_bytes("".join(f"{n}\t{l}\n" for n, l in TABLE).encode())
    (tmp_path / "a.pairs").write_bytes(_pairs(4000, 5))
    (tmp_path / "b.pairs").write_bytes(_pairs(3000, 6))
    (tmp_path / "f.bedpe").write_bytes(b"#chrom1\tstart1\tend1\tchrom2\tstart2\tend2\nchr1\t60000\t61000\tchr1\t90000\t91000\nchr1\t150000\t150500\tchr1\t120000\t121000\textra\n"
                                       b"chr2\t50000\t50100\tchr2\t70000\t70100\nchr1\t2000\t3000\tchr1\t249000\t250300\nchr1\t100000\t100000\tchr2\t60000\t60000\n")
    only = {"base": [*BALANCE, "--expected"], "apa": [*BALANCE, "--apa"], "pileup": [*BALANCE, "--pileup", str(tmp_path / "f.bedpe")], "saddle": [*BALANCE, "--saddle"],
            "insulation": [*BALANCE, "--insulation", "10000,25000"], "compare": [*BALANCE, "--compare", str(tmp_path / "b.pairs")], "viewpoint": ["--viewpoint", "chrV", "--vp-bin", "250"],
            "hic": [*BALANCE, "--hic"]}
    assert set(only) == set(PER_RES) == set(ONCE)
    every = [*BALANCE, "--expected", "--loops", "--apa", "--pileup", str(tmp_path / "f.bedpe"), "--eigs", "--saddle", "--insulation", "10000,25000",
             "--compare", str(tmp_path / "b.pairs"), "--viewpoint", "chrV", "--vp-bin", "250", "--hic"]

    def run(name, switches):
        os.makedirs(tmp_path / name)
        r = subprocess.run([EXE, "-g", str(tmp_path / "g.sizes"), "-r", ",".join(map(str, RES)), "-o", str(tmp_path / name / "o"), *switches, str(tmp_path / "a.pairs")],
                           stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=300)
        assert r.returncode == 0 and r.stdout == b"", (name, r.returncode, r.stderr[-2000:])
        return {f: open(tmp_path / name / f, "rb").read() for f in os.listdir(tmp_path / name)}, r.stderr

    got, warned = run("all", every)
    files = {k: [f"o.{r}.{e}" for r in RES for e in PER_RES[k]] + [f"o.{e}" for e in ONCE[k]] for k in only}
    assert sorted(got) == sorted(f for k in files for f in files[k])         # exactly the documented set
    assert len(got) == 13 * len(RES) + 15
    warnings = []
    for k in only:
        alone, w = run(k, only[k])
        warnings.append(w)
        assert set(files[k]) <= set(alone), (k, sorted(alone))
        for f in files[k]:
            assert got[f] == alone[f], (k, f)
    # the inputs are not degenerate: something was binned, skipped, balanced, scored and profiled, and one partial last bin is there
    stat = dict(ln.split(b"\t") for ln in got["o.matrix.stat"].splitlines())
    assert int(stat[b"Pairs"]) == 4000 and int(stat[b"Skipped"]) >= 40 and int(stat[b"nnz.1000"]) > int(stat[b"nnz.5000"]) > 500
    assert got["o.5000.bins.bed"].endswith(b"chrV\t15000\t17250\n") and b"chr1\t250000\t250300\n" in got["o.1000.bins.bed"]
    assert b"nan" not in got["o.5000.weights.bed"].split(b"\n")[3] and got["o.5000.insulation.tsv"].count(b"\n") == 1 + 51 + 25 + 4
    assert got["o.5000.eigs.tsv"].count(b"\n") == 1 + 80 and got["o.5000.saddle.tsv"].count(b"\n") == 1 + 50 * 51 // 2
    assert got["o.5000.apa.tsv"].count(b"\n") == 1 + 21 * 21 == got["o.1000.pileup.tsv"].count(b"\n") and got["o.pileup.stat"].startswith(b"5000\t5\t")
    assert got["o.scc.stat"].count(b"\n") == 2 * 4 and got["o.viewpoint.bedgraph"].count(b"\n") > 10 and got["o.hic"][:4] == b"HIC\0"
    assert set(warned.splitlines()) == {ln for w in warnings for ln in w.splitlines()}      # the same warnings, if any
