"""Pair statistics on the GPU (mkt_pairstat_* of include/mkt.h, microcket_amd.PairStats, bin/pairsstat): counters, dist_freq,
chrom_freq, the float64 bit patterns of area and P(s) and the bytes of both texts equal the definition (tests/pairstatdef.py) on every
directed family of tests/pairstat_cases.py, by every route (host pieces, device text, a context's key list, the executable), on every
call and in another process; the reference's cis0 / cis1K / cis10K / trans of the 36 golden cases come out of the kernel."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import microcket_amd as m
import pairstat_cases as pc
import pairstatdef as pd
import px2_inputs
import util

pytestmark = pytest.mark.gpu

EXE = os.path.join(os.path.dirname(m.lib_path()), "bin", "pairsstat")
INFO_KEYS = ("total", "skipped", "counted", "cis", "trans", "no_strand", "header_lines", "cis0", "cis1K", "cis10K", "ref_trans", "convergence_dist") + pd.GE_KEYS
_cache = {}


def family(name):
    """(family, the definition's result), made once and left unchanged"""
    if not _cache:
        for f in pc.families():
            _cache[f["name"]] = [f, None]
    e = _cache[name]
    if e[1] is None:
        f = e[0]
        e[1] = pd.stats(f["table"], f["text"], f["tol_permille"], f["min_count"])
    return e


NAMES = [f["name"] for f in pc.families()]


def table_for(text: bytes) -> bytes:
    names = sorted({f for ln in text.split(b"\n") if ln and not ln.startswith(b"#") for f in (ln.split(b"\t")[1], ln.split(b"\t")[3]) if len(f) <= 63} | {b"chr1"})
    return b"".join(n + b"\t4294967295\n" for n in names)


def bits(a):
    return np.asarray(a, dtype=np.float64).view(np.uint64).tolist()


def check(ps, info, want, name=""):
    assert {k: info[k] for k in INFO_KEYS} == {k: want.info[k] for k in INFO_KEYS}, name
    assert ps.dist_freq.tolist() == want.dist, name
    assert ps.chrom_freq.tolist() == want.chrom, name
    s = ps.scaling
    assert s.edges.tolist() == pd.EDGES + [pd.LAST_HI] and bits(s.area) == bits(want.area_f) and bits(s.P) == bits(want.P), name
    assert ps.stat_text() == want.stat_text and ps.scaling_text() == want.scaling_text, name


def run_text(f, piece=None):
    with m.PairStats(f["table"], device=0) as ps:
        text = f["text"]
        if piece is None:
            ps.add(text)
        else:
            for k in range(0, len(text), piece):
                ps.add(text[k:k + piece])
        info = ps.run(tol_permille=f["tol_permille"], min_count=f["min_count"])
        return info, ps.dist_freq.tolist(), ps.chrom_freq.tolist(), bits(ps.scaling.P), ps.stat_text(), ps.scaling_text(), ps.timing_ms()


@pytest.mark.parametrize("name", NAMES)
def test_every_family_equals_the_definition(name):
    f, want = family(name)
    with m.PairStats(f["table"], device=0) as ps:
        ps.add(f["text"])
        check(ps, ps.run(tol_permille=f["tol_permille"], min_count=f["min_count"]), want, name)
        t = ps.timing_ms()
        assert set(t) == {"index", "kernel", "total"} and all(v >= 0 for v in t.values())


@pytest.mark.parametrize("name,piece", [("strands", 1), ("skips", 1), ("wave_64_pairs", 1), ("edges", 7), ("lines_257", 7), ("edges", 4096), ("lines_4097", 4096), ("convergence_tol25_min40", 4096)])
def test_any_chunking_of_add_gives_the_same_results(name, piece):
    f, want = family(name)
    with m.PairStats(f["table"], device=0) as ps:
        for k in range(0, len(f["text"]), piece):
            ps.add(f["text"][k:k + piece])
        check(ps, ps.run(tol_permille=f["tol_permille"], min_count=f["min_count"]), want, (name, piece))


def test_more_text_after_a_run_and_other_options():
    f, want = family("convergence_tol25_min40")
    g, _ = family("strands")
    with m.PairStats(f["table"], device=0) as ps:
        with pytest.raises(m.MktError, match="before a run"):
            ps.stat_text()
        ps.add(f["text"])
        check(ps, ps.run(25, 40), want)
        for name in ("convergence_tol24_min40", "convergence_tol750_min40", "convergence_tol25_min39", "convergence_tol0_min0"):
            h, w = family(name)
            check(ps, ps.run(h["tol_permille"], h["min_count"]), w, name)
        ps.add(g["text"])                                                            # the next run reports everything seen so far
        check(ps, ps.run(25, 40), pd.stats(f["table"], f["text"] + g["text"], 25, 40), "more")


def test_device_text_of_a_bgzf_reader_gives_the_same_results():
    text = px2_inputs.case("blocks_many_bins")["text"]
    table = table_for(text)
    want = pd.stats(table, text, 50, 10)
    assert want.info["total"] > 1000 and want.info["header_lines"] == 2
    with m.PairsGz() as g:
        g.add(text)
        g.run()
        gz = g.gz_bytes()
    assert len(text) > 3 * 65280                                                     # several BGZF blocks
    with m.BgzfReader(device=0) as z, m.PairStats(table, device=0) as ps:
        z.add(gz)
        z.run()
        d, n = z.device_text()
        assert n == len(text)
        ps.add_device(d, n)
        check(ps, ps.run(50, 10), want, "whole")
    with m.BgzfReader(device=0) as z, m.PairStats(table, device=0) as ps:           # in three pieces cut inside lines, host text between
        z.add(gz)
        z.run()
        d, n = z.device_text()
        a, b = n // 3 + 5, 2 * n // 3 + 11
        ps.add(text[:17])
        ps.add_device(d + 17, a - 17)
        ps.add_device(d + a, b - a)
        ps.add_device(d + b, n - b)
        check(ps, ps.run(50, 10), want, "pieces")


def golden_cases():
    with open(os.path.join(util.GOLDEN, "golden.json")) as f:
        g = json.load(f)
    return [(i["name"], c) for i in g["inputs"] for c in i["cases"] if "pairs_sorted" in c]


def test_reference_pin_on_the_golden_pairs():
    cases = golden_cases()
    assert len(cases) == 36
    for name, c in cases:
        text = c["pairs_sorted"].encode()
        with m.PairStats(table_for(text), device=0) as ps:
            ps.add(text)
            info = ps.run()
        log = dict(ln.split("\t") for ln in c["log"].splitlines())
        got = {"trans": info["ref_trans"], "cis10K": info["cis10K"], "cis1K": info["cis1K"], "cis0": info["cis0"]}
        assert {k: str(v) for k, v in got.items()} == {k: log[k] for k in got}, (name, c["mode"])
        assert info["total"] == c["pairs_lines"]


@pytest.mark.parametrize("k", range(len(pc.MALFORMED)))
def test_malformed_lines_are_refused_with_their_number(k):
    text, number = pc.MALFORMED[k]
    for piece in (None, 5):
        with m.PairStats(pc.TABLE, device=0) as ps:
            if piece is None:
                ps.add(text)
            else:
                for j in range(0, len(text), piece):
                    ps.add(text[j:j + piece])
            with pytest.raises(m.MktError, match=rf"file refused: line {number}:"):
                ps.run()


def test_table_of_2048_names_is_taken_and_2049_refused():
    with m.PairStats(pc.name_table(2048), device=0) as ps:
        ps.add(b"a\tc7\t5\tc2047\t9\t+\t-\nb\tc2047\t3047\tc2047\t1\t-\t-\nc\tc2047\t3048\tc2047\t1\t-\t-\n")
        info = ps.run()
        assert (info["total"], info["skipped"], info["cis"], info["trans"]) == (3, 1, 1, 1)
        cf = ps.chrom_freq
        assert cf.shape == (2048, 2048) and cf[7, 2047] == 1 and cf[2047, 2047] == 1 and int(cf.sum()) == 2
    with pytest.raises(m.MktError, match="out of range.*2049 names.*2048"):
        m.PairStats(pc.name_table(2049), device=0)
    with pytest.raises(m.MktError, match="bad argument"):
        m.PairStats(b"chr1\n", device=0)
    with pytest.raises(m.MktError, match="twice"):
        m.PairStats(b"chr1\t5\nchr1\t6\n", device=0)


# ---- the key route ------------------------------------------------------------------------------------------------------------------
HG38 = b"".join(n + b"\t%d\n" % L for n, L in (
    (b"chr1", 248956422), (b"chr10", 133797422), (b"chr11", 135086622), (b"chr12", 133275309), (b"chr13", 114364328), (b"chr14", 107043718), (b"chr15", 101991189),
    (b"chr16", 90338345), (b"chr17", 83257441), (b"chr18", 80373285), (b"chr19", 58617616), (b"chr2", 242193529), (b"chr20", 64444167), (b"chr21", 46709983),
    (b"chr22", 50818468), (b"chr3", 198295559), (b"chr4", 190214555), (b"chr5", 181538259), (b"chr6", 170805979), (b"chr7", 159345973), (b"chr8", 145138636),
    (b"chr9", 138394717), (b"chrM", 16569), (b"chrX", 156040895)))                    # (no chrY: its pairs are skipped)


def test_keys_of_a_context_equal_the_text_route():
    sam = util.synth("unc", 61, 6000)
    with m.Context("unc", 0.5, 10, False, 4, device=0, block_bytes=1 << 20, ordered=True, extensions=m.EXT_KEYS) as c:
        pairs, _s, st, _log = c.run_bytes(sam, chunk=1 << 20)
        n = pairs.count(b"\n")
        assert n == st.pairs and n >= 1500
        total, dups, flags = c.ext_dedup(True)
        assert total == n and len(flags) == n
        if not any(flags):
            flags = bytes(1 if k % 7 == 3 else 0 for k in range(n))                 # any flags do: they only have to leave lines out
        for fl in (None, flags):
            want = pd.stats(HG38, pairs, 50, 100, skip=fl)
            with m.PairStats(HG38, device=0) as ps:
                ps.add_keys(c, True, fl)
                check(ps, ps.run(50, 100), want, fl is not None)
        # without drop_last the list may hold the pair of the input's last group, which the context did not print (quirk Q1 of mkt_finish)
        want = pd.stats(HG38, pairs, 50, 100)
        with m.PairStats(HG38, device=0) as ps:
            ps.add_keys(c, False)
            info = ps.run(50, 100)
            extra = info["total"] - want.info["total"]
            assert extra in (0, 1)
            if extra == 0:
                check(ps, info, want, "all keys")
            else:
                assert int(ps.chrom_freq.sum()) + info["skipped"] == n + 1 and (ps.chrom_freq >= np.array(want.chrom, dtype=np.uint64)).all()
                assert (ps.dist_freq >= np.array(want.dist, dtype=np.uint64)).all() and int(ps.dist_freq.sum()) - sum(map(sum, want.dist)) in (0, 1)
        kept = b"".join(ln for ln, f in zip(pairs.splitlines(keepends=True), flags) if not f)
        want = pd.stats(HG38, kept, 50, 100)
        assert want.info["skipped"] > 0 or b"chrY" not in pairs
        with m.PairStats(HG38, device=0) as ps:                                      # ... and the text route on the lines that stay
            ps.add(kept)
            check(ps, ps.run(50, 100), want, "text")
        with m.PairStats(HG38, device=0) as ps:
            with pytest.raises(m.MktError, match="flags"):
                ps.add_keys(c, True, flags[:-1])
    with m.Context("unc", 0.5, 10, False, 4, device=0) as c3, m.PairStats(HG38, device=0) as ps:       # a context without the key list
        with pytest.raises(m.MktError, match="MKT_EXT_KEYS"):
            ps.add_keys(c3, True)


# ---- the executable -------------------------------------------------------------------------------------------------------------------
def _cli(args, stdin=None):
    return subprocess.run([EXE, *args], input=stdin, stdout=subprocess.PIPE, stderr=subprocess.PIPE)


def test_cli_on_a_file_on_stdin_and_on_a_gz(tmp_path):
    f, want = family("edges")
    ft, fp = tmp_path / "chrom.sizes", tmp_path / "final.pairs"
    ft.write_bytes(f["table"])
    fp.write_bytes(f["text"])
    r = _cli(["-g", str(ft), str(fp)])
    assert r.returncode == 0 and r.stdout == want.stat_text, r.stderr.decode()
    r = _cli(["-g", str(ft), "-o", str(tmp_path / "out"), "-"], stdin=f["text"])
    assert r.returncode == 0 and r.stdout == b"", r.stderr.decode()
    assert (tmp_path / "out.pairs.stat").read_bytes() == want.stat_text and (tmp_path / "out.scaling.tsv").read_bytes() == want.scaling_text
    h, w = family("convergence_tol24_min40")
    fp.write_bytes(h["text"])
    r = _cli(["-g", str(ft), "--tol", "24", "--min-count", "40", str(fp)])
    assert r.returncode == 0 and r.stdout == w.stat_text and b"summary/convergence_dist\t1000\n" in r.stdout
    text = px2_inputs.case("blocks_many_bins")["text"]
    (tmp_path / "t2").write_bytes(table_for(text))
    with m.PairsGz() as g:
        g.add(text)
        g.run()
        g.write(tmp_path / "final.pairs.gz")
    wz = pd.stats(table_for(text), text)
    r = _cli(["-g", str(tmp_path / "t2"), "-o", str(tmp_path / "z"), str(tmp_path / "final.pairs.gz")])
    assert r.returncode == 0, r.stderr.decode()
    assert (tmp_path / "z.pairs.stat").read_bytes() == wz.stat_text and (tmp_path / "z.scaling.tsv").read_bytes() == wz.scaling_text
    # refusals
    assert _cli([]).returncode == 2 and _cli(["-g", str(ft)]).returncode == 2
    assert _cli(["-g", str(tmp_path / "none"), str(fp)]).returncode == 10 and _cli(["-g", str(ft), str(tmp_path / "none")]).returncode == 10
    fp.write_bytes(pc.MALFORMED[0][0])
    r = _cli(["-g", str(ft), str(fp)])
    assert r.returncode == 12 and b"line 2:" in r.stderr and r.stdout == b""
    (tmp_path / "big").write_bytes(pc.name_table(2049))
    r = _cli(["-g", str(tmp_path / "big"), str(fp)])
    assert r.returncode == 12 and b"2048" in r.stderr


def test_two_runs_in_one_process_and_a_second_process_give_the_same_bytes(tmp_path):
    f, want = family("lines_4097")
    a, b = run_text(f), run_text(f, piece=1000)
    assert a[:6] == b[:6] and a[4] == want.stat_text and a[5] == want.scaling_text
    ft, fp = tmp_path / "chrom.sizes", tmp_path / "final.pairs"
    ft.write_bytes(f["table"])
    fp.write_bytes(f["text"])
    code = ("import sys; sys.path.insert(0, %r); import microcket_amd as m\n"
            "ps = m.PairStats(open(%r, 'rb').read()); ps.add(open(%r, 'rb').read()); ps.run(%d, %d)\n"
            "sys.stdout.buffer.write(ps.stat_text() + b'\\0' + ps.scaling_text())\n") % (util.ROOT, str(ft), str(fp), f["tol_permille"], f["min_count"])
    r = subprocess.run([sys.executable, "-c", code], stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    assert r.returncode == 0, r.stderr.decode()[-2000:]
    assert r.stdout == want.stat_text + b"\0" + want.scaling_text
