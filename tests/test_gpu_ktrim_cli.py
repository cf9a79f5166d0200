"""bin/ktrim on the GPU: the reference's argv forms and exit codes, -c and the two files without it, PREFIX.trim.log byte for byte
against the goldens made by Ktrim 1.6.0 (tests/golden/ktrim_golden.json), and the driver's `ktrim -c | krmdup.pipe` with this
project's two drop-ins against the hashes of the reference's own pipe.  Every child process runs under its own time limit."""
import os
import subprocess

import pytest

import ktrim_cases as kc
import ktrimdef as kd
import microcket_amd as m
import util
from test_ktrim_def import batch_input, batch_output, case_input, golden

pytestmark = pytest.mark.gpu
BIN = os.path.dirname(m.exe_path())
EXE = os.path.join(BIN, "ktrim")
KRMDUP_PIPE = os.path.join(BIN, "krmdup.pipe")
LIMIT = 120


def _need_gpu():
    if m.device_count() < 1:
        pytest.fail("no HIP device")


def run(tmp_path, t1, t2, argv=(), c=True, env=None, names=("a.fq", "b.fq")):
    """-> (rc, stdout, stderr, {file name behind the prefix: bytes})"""
    for n, t in zip(names, (t1, t2)):
        if t is not None:
            (tmp_path / n).write_bytes(t)
    p = subprocess.run([EXE, "-t", "4", "-o", "o", "-1", names[0], "-2", names[1], *(("-c",) if c else ()), *argv], cwd=tmp_path, stdout=subprocess.PIPE,
                       stderr=subprocess.PIPE, timeout=LIMIT, env=dict(os.environ, **(env or {})))
    files = {f[2:]: (tmp_path / f).read_bytes() for f in os.listdir(tmp_path) if f.startswith("o.")}
    return p.returncode, p.stdout, p.stderr.decode(), files


def test_stdout_and_log_on_goldens(tmp_path):
    _need_gpu()
    for c in golden()["cases"][:3]:
        rc, out, err, files = run(tmp_path, *case_input(c), c["argv"], env={"MKT_TRIM_SEGMENT_PAIRS": "1000"})
        assert rc == 0 and kd.sha(out) == c["stdout_sha256"] and files == {"trim.log": c["log"].encode()}, (c["name"], err)
    for b in golden()["batches"]:
        if b["name"] in ("length_grid", "quality_wmax", "mismatch_limit_m0.3", "custom_different", "text", "adapter_position_bgi"):
            rc, out, err, files = run(tmp_path, *batch_input(b), b["argv"])
            assert rc == 0 and out == batch_output(b) and files["trim.log"] == b["log"].encode(), (b["name"], err)


def test_files_without_c(tmp_path):
    _need_gpu()
    c = golden()["cases"][0]
    rc, out, err, files = run(tmp_path, *case_input(c), c=False)
    assert rc == 0 and out == b"" and sorted(files) == ["read1.fq", "read2.fq", "trim.log"], err
    assert (kd.sha(files["read1.fq"]), kd.sha(files["read2.fq"]), files["trim.log"].decode()) == (c["read1_sha256"], c["read2_sha256"], c["log"])


def test_file_lists_and_stdin(tmp_path):
    _need_gpu()
    b = next(x for x in golden()["batches"] if x["name"] == "decoy_seeds")
    t1, t2 = batch_input(b)
    want = batch_output(b)
    (tmp_path / "c.fq").write_bytes(t1[:-1])      # the first file of the list without its final newline
    (tmp_path / "d.fq").write_bytes(t2)
    (tmp_path / "a.fq").write_bytes(t1)
    (tmp_path / "b.fq").write_bytes(t2)
    rc, out, err, files = run(tmp_path, None, None, names=("c.fq,a.fq", "d.fq,b.fq"))
    assert rc == 0 and out == want + want, err
    assert files["trim.log"].decode() == kd.log_text(kd.trim_stream(t1 + t1, t2 + t2)[3])
    p = subprocess.run([EXE, "-o", "o", "-1", "/dev/stdin", "-2", "b.fq", "-c"], cwd=tmp_path, input=t1, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=LIMIT)
    assert p.returncode == 0 and p.stdout == want, p.stderr.decode()
    assert run(tmp_path, None, None, names=("a.fq,c.fq", "b.fq"))[0] == 110


def test_exit_codes(tmp_path):
    _need_gpu()
    t1, t2 = kc.text_of([kc.pair("x", 60, 100)])
    for argv, code in ((["-q", "0"], 12), (["-p", "0"], 12), (["-w", "0"], 12), (["-s", "9"], 11), (["-k", "foo"], 13), (["-a", "ACGTACG"], 20), (["-b", "ACGTACGTAA"], 14),
                       (["-z"], 2), (["-U", "a.fq"], 15), (["-f", "list"], 15), (["-R"], 15), (["-k", "CLIP"], 15), (["-m", "2"], 1)):
        rc, out, err, files = run(tmp_path, t1, t2, argv)
        assert rc == code and out == b"" and err, (argv, rc, err)
    assert run(tmp_path, t1, t2, ["-s", "10"])[0] == 0
    for argv, code in ((["-h"], 0), (["-v"], 0), (["-1", "a.fq", "-2", "b.fq", "-c"], 3), (["-o", "o", "-2", "b.fq"], 2), (["-o", "o", "-1", "a.fq"], 15),
                       (["-o", "o", "-1", "a.fq.gz", "-2", "b.fq"], 15), (["-o", "o", "-1", "missing.fq", "-2", "b.fq", "-c"], 104)):
        p = subprocess.run([EXE, *argv], cwd=tmp_path, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=LIMIT)
        assert p.returncode == code, (argv, p.returncode, p.stderr.decode())
    rc, out, err, files = run(tmp_path, t1, t2, ["-k", "nextera", "-a", "ACGTACGTAC"])      # the kit wins, with a warning
    assert rc == 0 and "Warning" in err and out == kd.trim_stream(t1, t2, kit="nextera")[0]


@pytest.mark.parametrize("name", ["qual_short", "header_200", "read_511", "lines_not_4", "pair_counts"])
def test_refused_input(tmp_path, name):
    _need_gpu()
    _, t1, t2, opts, what = next(r for r in kc.REFUSED_INPUT if r[0] == name)
    rc, out, err, files = run(tmp_path, t1, t2)
    assert rc == 121 and what in err, err


def test_pipe_into_krmdup(tmp_path):
    """bin/ktrim -c | bin/krmdup.pipe -i /dev/stdin -o o.rmdup: the products of the reference's own pipe"""
    _need_gpu()
    g = golden()["pipe"]
    t1, t2 = case_input(g)
    (tmp_path / "a.fq").write_bytes(t1)
    (tmp_path / "b.fq").write_bytes(t2)
    k = subprocess.Popen([EXE, "-t", "4", "-o", "o", "-1", "a.fq", "-2", "b.fq", "-c"], cwd=tmp_path, stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    r = subprocess.Popen([KRMDUP_PIPE, "-i", "/dev/stdin", "-o", "o.rmdup"], cwd=tmp_path, stdin=k.stdout, stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    k.stdout.close()
    out, err = r.communicate(timeout=LIMIT)
    kerr = k.stderr.read().decode()
    assert k.wait(timeout=LIMIT) == 0 and r.returncode == 0, (kerr, err.decode())
    prod = {"stdout_records": b"\n".join(util.fastq_records(out)), "trim.log": (tmp_path / "o.trim.log").read_bytes()}
    for f in sorted(os.listdir(tmp_path)):
        if f.startswith("o.rmdup"):
            prod[f[2:]] = (tmp_path / f).read_bytes()
    assert {n: kd.sha(v) for n, v in prod.items()} == g["products"]
