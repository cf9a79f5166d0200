"""Read stitching without a GPU: the definition (tests/stitchdef.py) against the golden vectors made by the program it restates
(tests/golden/stitch_golden.json: FLASH v1.2.11 with one combiner thread + deal.flash.pl) and, where that program is present,
against a live run on a fresh seed; the host side of bin/stitch and of the C ABI (argument check, limits)."""
import json
import os
import re
import subprocess

import pytest

import microcket_amd as m
import stitchdef as sd

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF_FLASH = "/root/reference/bin/flash"
_cache = {}


def golden():
    if "g" not in _cache:
        with open(os.path.join(ROOT, "tests", "golden", "stitch_golden.json")) as f:
            _cache["g"] = json.load(f)
    return _cache["g"]


def case_kw(c):
    """the arguments of a golden case as stitchdef.stitch / Stitcher take them"""
    a, d = c["flash_args"], {"-m": 10, "-M": 150, "-x": 0.25}
    for k in range(0, len(a), 2):
        d[a[k]] = float(a[k + 1]) if a[k] == "-x" else int(a[k + 1])
    kw = dict(m=d["-m"], M=d["-M"], x=d["-x"])
    if c["deal_args"]:
        kw.update(cut_tail=int(c["deal_args"][0]), min_size=int(c["deal_args"][1]))
    return kw


def case_input(c):
    """the input of a golden case and the definition's result for it, made once and shared (never modified)"""
    key = ("case", c["name"])
    if key not in _cache:
        text = sd.synth(c["seed"], c["pairs"], c["read_len"])
        _cache[key] = (text, sd.stitch(text, **case_kw(c)))
    return _cache[key]


def edge_text(e):
    h1, s1, q1, h2, s2, q2 = e["input"]
    return f"@{h1}\n{s1}\n+\n{q1}\n@{h2}\n{s2}\n+\n{q2}\n".encode()


def edge_set():
    """all edge pairs as one input, and the program's outputs for them in input order"""
    E = golden()["edges"]
    text = b"".join(edge_text(e) for e in E)
    want = {k: "".join(e[k] for e in E).encode() for k in ("tab", "ext", "cut1", "cut2")}
    comb = sum(1 for e in E if e["tab"].count("\t") == 2)
    passed = sum(1 for e in E if e["cut1"])
    want["stat"] = b"Combined\t%d\tUncombined\t%d\tPass\t%d\n" % (comb, len(E) - comb, passed)
    return text, want


def test_definition_reproduces_every_edge_line():
    E = golden()["edges"]
    assert len(E) >= 40
    for e in E:
        r = sd.stitch(edge_text(e))
        for k in ("tab", "ext", "cut1", "cut2", "stat"):
            assert r[k].decode() == e[k], (e["name"], k)
    text, want = edge_set()
    r = sd.stitch(text)
    for k in want:
        assert r[k] == want[k], k
    kinds = {e["name"]: e["tab"].count("\t") for e in E}
    assert kinds["full_160_mm37"] == 2 and kinds["full_160_mm38"] == 4          # the min(eff, M) cap: 38 / 160 < 0.25 < 38 / 150
    assert kinds["n_eff_10"] == 2 and kinds["n_eff_9"] == 4 and kinds["len9"] == 4 and kinds["len10_overlap10"] == 2


@pytest.mark.parametrize("name", [c["name"] for c in json.load(open(os.path.join(ROOT, "tests", "golden", "stitch_golden.json")))["cases"]])
def test_definition_reproduces_every_hash(name):
    c = next(c for c in golden()["cases"] if c["name"] == name)
    text, r = case_input(c)
    assert sd.sha(text) == c["input_sha256"]                     # the generator
    comb, unc = sd.by_kind(r["tab"])
    assert sd.sha(comb) == c["tab_combined_sha256"] and sd.sha(unc) == c["tab_uncombined_sha256"]
    assert sd.sha(r["ext"]) == c["ext_sha256"] and sd.sha(r["cut1"]) == c["cut1_sha256"] and sd.sha(r["cut2"]) == c["cut2_sha256"]
    assert r["stat"].decode() == c["stat"] and r["percent"] == c["percent"]
    assert r["total"] == c["pairs"] and 0 < r["combined"] < r["total"]


@pytest.mark.skipif(not os.path.exists(REF_FLASH), reason="the reference's bin/flash is not on this machine")
def test_definition_equals_the_program_on_a_fresh_seed():
    """Every line of the program's output, none excluded.  Its stream alternates between blocks of combined and of uncombined lines
    (stitchdef.by_kind), so the lines are compared kind by kind, in order, and as a whole multiset."""
    seed = int.from_bytes(os.urandom(4), "little")
    text = sd.synth(seed, 4000)
    p = subprocess.run([REF_FLASH, "-q", "--interleaved-input", "-m", "10", "-M", "150", "-t", "1", "-To", "-c", "-"], input=text, stdout=subprocess.PIPE,
                       stderr=subprocess.PIPE)
    assert p.returncode == 0, p.stderr
    r = sd.stitch(text)
    assert sd.by_kind(p.stdout) == sd.by_kind(r["tab"]), seed
    assert sorted(p.stdout.split(b"\n")) == sorted(r["tab"].split(b"\n")), seed
    assert p.stdout.count(b"\n") == 4000


def test_definition_refuses_what_the_abi_refuses():
    rec = lambda n1, n2=30, q="I": b"@a/1\n%s\n+\n%s\n@a/2\n%s\n+\n%s\n" % (b"A" * n1, q.encode() * n1, b"C" * n2, b"I" * n2)
    assert sd.stitch(rec(sd.MAX_READ))["total"] == 1
    for bad in (rec(sd.MAX_READ + 1), rec(0), rec(30, 0), rec(30)[:-20], rec(30, q=" "), rec(30) + b"@x\nAC\n"):
        with pytest.raises(ValueError):
            sd.stitch(bad)
    with pytest.raises(ValueError):
        sd.stitch(rec(30), M=sd.MAX_M + 1)
    recq = lambda c: b"@a/1\n%s\n+\n%s\n@a/2\n%s\n+\n%s\n" % (b"A" * 30, bytes([c]) * 30, b"C" * 30, bytes([c]) * 30)
    for phred in (33, 64):                                        # a quality byte: phred_offset .. phred_offset + 93, for any offset
        assert sd.stitch(recq(phred), phred=phred)["total"] == 1 and sd.stitch(recq(phred + 93), phred=phred)["total"] == 1
        for c in (phred - 1, phred + 94):
            with pytest.raises(ValueError):
                sd.stitch(recq(c), phred=phred)
    hdr =open(os.path.join(ROOT, "include", "mkt.h")).read()
    assert int(re.search(r"#define MKT_STITCH_MAX_READ (\d+)", hdr).group(1)) == sd.MAX_READ == m.capi.STITCH_MAX_READ >= 512
    assert int(re.search(r"#define MKT_STITCH_MAX_M (\d+)", hdr).group(1)) == sd.MAX_M == m.capi.STITCH_MAX_M


def test_float32_and_integer_comparisons_agree_up_to_max_m():
    """The range stated in include/mkt.h.  Two different fractions with denominators <= M differ by at least 1 / M^2; rounding to
    float32 keeps them apart and in order when that exceeds the float32 step at their size.  Densities that can decide are below 2,
    quality scores below 93 * 2 (step 2^-16): M = MAX_M = 255 is the largest M with 1 / M^2 > 2^-16.  The densities are also checked
    exhaustively: the float32 quotients order exactly as the cross-multiplied integers."""
    import numpy as np
    M = sd.MAX_M
    assert float(np.spacing(np.float32(93 * 2 - 0.001))) < 1.0 / (M * M) and not float(np.spacing(np.float32(93 * 2 - 0.001))) < 1.0 / ((M + 1) * (M + 1))
    assert float(np.spacing(np.float32(1.999))) < 1.0 / (M * M)
    sl = np.arange(1, M + 1, dtype=np.int64)
    num = np.arange(0, 2 * M + 1, dtype=np.int64)
    v = (num[:, None].astype(np.float32) / sl[None, :].astype(np.float32)).ravel()
    n2, s2 = np.broadcast_to(num[:, None], (len(num), M)).ravel(), np.broadcast_to(sl[None, :], (len(num), M)).ravel()
    keep = n2 < 2 * s2
    v, n2, s2 = v[keep], n2[keep], s2[keep]
    order = np.argsort(v, kind="stable")
    v, n2, s2 = v[order], n2[order], s2[order]
    assert np.array_equal(v[1:] == v[:-1], n2[1:] * s2[:-1] == n2[:-1] * s2[1:])      # equal as float32 exactly when equal as fractions
    assert np.all(n2[1:] * s2[:-1] >= n2[:-1] * s2[1:])                                # and sorted by float32 is sorted as fractions


def _exe():
    from microcket_amd import build
    if not os.path.exists(m.lib_path()):
        build.build_lib()
    return build.build_stitch()


def test_stitch_executable_arguments_without_gpu(tmp_path):
    exe = _exe()
    fq = tmp_path / "x.fq"
    fq.write_bytes(sd.synth(1, 5))
    run = lambda *a: subprocess.run([exe, *a], stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    r = run()
    assert r.returncode == 2 and b"Usage" in r.stderr
    assert run(str(fq)).returncode == 2                                            # neither -o nor --tab
    assert run("-o", str(tmp_path / "o")).returncode == 2                          # no input
    assert run("-o", str(tmp_path / "o"), str(fq), "extra").returncode == 2
    r = run("-M", str(sd.MAX_M + 1), "-o", str(tmp_path / "o"), str(fq))
    assert r.returncode == 1 and b"max overlap" in r.stderr and not (tmp_path / "o.ext.fq").exists()
    r = run("-m", "0", "--tab", str(fq))
    assert r.returncode == 1 and b"min overlap" in r.stderr
    assert run("-m", "200", "--tab", str(fq)).returncode == 1                      # above -M
    assert run("-x", "1.5", "--tab", str(fq)).returncode == 1
    assert run("-m", "ten", "--tab", str(fq)).returncode == 1
    assert run("--cut-tail", "70000", "--tab", str(fq)).returncode == 1
    assert run("--tab", str(tmp_path / "missing.fq")).returncode == 10
    assert run("-o", str(tmp_path / "nodir" / "o"), str(fq)).returncode == 11
    if m.device_count() == 0:
        r = run("--tab", "--cut-tail", "5", "--min-size", "30", "-p", "33", "-x", "0.1", "-m", "15", "-M", "80", str(fq))
        assert r.returncode == 20 and r.stdout == b""                              # every option parsed; no GPU: loud failure, no output


def test_stitch_check_is_the_abi_argument_check():
    _exe()
    assert m.stitch_check() is None and m.stitch_check(1, sd.MAX_M, 1.0, 0, 0, 0) is None
    assert "max overlap" in m.stitch_check(max_overlap=sd.MAX_M + 1)
    assert "min overlap" in m.stitch_check(min_overlap=0) and "min overlap" in m.stitch_check(min_overlap=151)
    assert "density" in m.stitch_check(max_mismatch_density=-0.1) and "density" in m.stitch_check(max_mismatch_density=float("nan"))
    assert "phred" in m.stitch_check(phred_offset=128)
    assert "cut tail" in m.stitch_check(cut_tail=1 << 16)
