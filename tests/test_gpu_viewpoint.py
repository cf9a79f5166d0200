"""Viewpoint contact profiles on the GPU (mkt_matrix_viewpoint, Matrix.viewpoint, pairs2matrix --viewpoint / --ebv).
 * tests/golden/viewpoint_golden.json holds what the reference's two Perl scripts (util/analyze.EBV) wrote for the seeded inputs of
   tests/viewpoint_inputs.py: the texts made from the GPU's arrays, and the files of the executable, are those bytes.
 * Everything else is compared with tests/viewpointdef.py, the definition in plain Python.  All of it is integers: no tolerance."""
import ctypes as C
import os
import random
import subprocess

import numpy as np
import pytest

import microcket_amd as m
import util
import viewpoint_inputs as vi
import viewpointdef as vd

pytestmark = pytest.mark.gpu

EXE = os.path.join(util.ROOT, "microcket_amd", "bin", "pairs2matrix")
LDS_BINS = 8192                                                                   # kVpLdsBins of csrc/mkt_viewpoint.h


def _need_gpu():
    if m.device_count() < 1:
        pytest.fail("no HIP device")
    if not os.path.exists(EXE):
        from microcket_amd import build
        build.build_pairs2matrix()


def _loaded(ttext, text, pieces=0):
    mx = m.Matrix(ttext, [1000000], device=0)
    if pieces:
        for p in range(0, len(text), pieces):
            mx.add(text[p:p + pieces])
    else:
        mx.add(text)
    mx.run()
    return mx


def _as_profile(r):
    """the arrays of Matrix.viewpoint_result() in the shape of viewpointdef.Profile"""
    i = r.info
    return vd.Profile(i.total, list(zip(r.link_vbin.tolist(), r.link_chrom.tolist(), r.link_pbin.tolist(), r.link_count.tolist())), r.track.tolist(),
                      list(zip(r.partner_chrom.tolist(), r.partner_pbin.tolist(), r.partner_count.tolist())), i.partner_cells, i.min_loop, i.links_kept)


def _raw(mx):
    r = mx.viewpoint_result()
    return b"|".join(x.tobytes() for x in r[:8]) + repr(tuple(r.info)).encode()


def _check(label, mx, ttext, text, name, partners=None, **opts):
    """Matrix.viewpoint against the definition; returns the profile"""
    names, lens = vd.parse_table(ttext)
    v = names.index(name)
    want = vd.profile(vd.records(text, names, lens), names, v, vd.partner_set(names, v, partners) - {v}, **opts)
    info = mx.viewpoint(name, partners, **opts)
    got = _as_profile(mx.viewpoint_result())
    for f in vd.Profile._fields:
        assert getattr(got, f) == getattr(want, f), (label, opts, f, getattr(got, f), getattr(want, f))
    assert info.links == len(want.links) and info.viewpoint_bins == len(want.track) and info.partner_cells_kept == len(want.partners)
    assert all(a < b for a, b in zip(want.links, want.links[1:]))                                   # strictly ascending
    return got


# ---- 1. the reference's texts --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", range(len(vi.CASE_PARAMS)))
def test_goldens_through_the_binding(k):
    _need_gpu()
    c = vi.cases()[k]
    tt, text = vi.table_text(), vi.make(c["gen"])
    names, _ = vd.parse_table(tt)
    with _loaded(tt, text) as mx:
        o = dict(vbin=c["vbin"], second_side_only=1, origin=0, hotspot_ratio=c["ratio"])
        mx.viewpoint(vi.VIEWPOINT, vi.PARTNER_RE, pbin=c["pbin"], **o)
        a = _as_profile(mx.viewpoint_result())
        mx.viewpoint(vi.VIEWPOINT, vi.PARTNER_RE, pbin=c["track_bin"], min_count=c["min_count"], **o)
        b = _as_profile(mx.viewpoint_result())
    assert vd.track_text(a, vi.VIEWPOINT, c["vbin"]).decode() == c["bedgraph"]
    assert vd.links_text(a, names, c["vbin"], c["pbin"]).decode() == c["links"]
    assert vd.partners_text(b, names, c["track_bin"]).decode() == c["partners"]


@pytest.mark.parametrize("k", range(len(vi.CASE_PARAMS)))
def test_goldens_through_the_executable(tmp_path, k):
    _need_gpu()
    c = vi.cases()[k]
    (tmp_path / "g.sizes").write_bytes(vi.table_text())
    (tmp_path / "in.pairs").write_bytes(vi.make(c["gen"]))
    sub = ["--vp-bin", str(c["vbin"]), "--vp-partner-bin", str(c["pbin"]), "--vp-track-bin", str(c["track_bin"]), "--vp-min-count", str(c["min_count"]), "--vp-hotspot", repr(c["ratio"])]
    if c["name"] == "defaults":
        sub = ["--ebv"]                                                           # the preset alone: 200 / 1000000 / 1000 / 5 / 0.01
    elif k % 2:
        sub = ["--ebv"] + sub
    else:
        sub = ["--viewpoint", vi.VIEWPOINT, "--vp-partners", vi.PARTNER_RE, "--vp-second-side"] + sub
    r = subprocess.run([EXE, "-g", str(tmp_path / "g.sizes"), "-r", "1000000", "-o", str(tmp_path / "o"), *sub, str(tmp_path / "in.pairs")], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=300)
    assert r.returncode == 0, r.stderr
    assert open(tmp_path / "o.viewpoint.bedgraph").read() == c["bedgraph"]
    assert open(tmp_path / "o.viewpoint.links").read() == c["links"]
    assert open(tmp_path / "o.partners.bedgraph").read() == c["partners"]
    stat = dict(ln.split("\t") for ln in open(tmp_path / "o.viewpoint.stat").read().splitlines())
    assert stat["Viewpoint"] == vi.VIEWPOINT and stat["Skipped"] == "0" and int(stat["Total"]) == sum(int(ln.split("\t")[3]) for ln in c["bedgraph"].splitlines())


# ---- 2. shapes where the kernels can go wrong ---------------------------------------------------------------------------------------------
SMALL = [("chrA", 5000), ("chrV", 3000), ("chrB", 70000), ("chrC", 900)]


def _random_text(n, seed, table=SMALL, junk=True):
    """n lines: pairs in both orders between every two chromosomes, and (junk) skipped pairs and '#' lines among them"""
    rng = random.Random(seed)
    lens = dict(table)
    names = [t[0] for t in table]
    out = []
    for i in range(n):
        r = rng.random()
        a, b = rng.choice(names), rng.choice(names)
        if junk and r < 0.03:
            out.append("#comment\n")
        elif junk and r < 0.06:
            out.append(f"r{i}\tchrQ\t5\t{b}\t7\t+\t-\n")                          # unknown chromosome
        elif junk and r < 0.09:
            out.append(f"r{i}\t{a}\t{lens[a] + 1}\t{b}\t1\t+\t-\n")               # past the end
        elif junk and r < 0.11:
            out.append(f"r{i}\t{a}\t1\t{b}\t0\t+\t-\n")                           # position 0
        else:
            pa = rng.choice([1, lens[a], rng.randint(1, lens[a])])
            pb = rng.choice([1, lens[b], rng.randint(1, lens[b])])
            out.append(f"r{i}\t{a}\t{pa}\t{b}\t{pb}\t+\t-\n")
    return "".join(out).encode()


@pytest.mark.parametrize("n", [1, 63, 64, 65, 255, 256, 257, 100003])
def test_record_counts_origins_and_sides(n):
    _need_gpu()
    tt = vi.table_text(SMALL)
    text = _random_text(n, 100 + n) if n > 1 else b"r0\tchrB\t70000\tchrV\t3000\t+\t-\n"
    with _loaded(tt, text) as mx:
        for origin in (0, 1):
            for sso in (0, 1):
                p = _check(f"n {n}", mx, tt, text, "chrV", None, vbin=7, pbin=13, origin=origin, second_side_only=sso, min_count=1 + (n > 1000), hotspot_ratio=0.3)
        if n >= 255:
            assert p.total > 0
        _check(f"n {n}, list", mx, tt, text, "chrV", ["chrC", "chrA"], vbin=200, pbin=1000)
        _check(f"n {n}, regex", mx, tt, text, "chrB", "r[AV]$", vbin=1000, pbin=100, origin=1)
        s, t = mx.viewpoint_timing_ms()
        assert s > 0 and t >= 0


def test_nothing_everything_sparse_and_one_cell():
    _need_gpu()
    tt = vi.table_text(SMALL)
    hit, miss = b"x\tchrA\t17\tchrV\t900\t+\t-\n", b"x\tchrA\t17\tchrC\t90\t+\t-\n"
    with _loaded(tt, miss * 3000) as mx:                                          # no record matches
        p = _check("nothing", mx, tt, miss * 3000, "chrV")
        assert p.total == 0 and p.links == [] and p.track == [] and p.partners == [] and p.min_loop == 0
    with _loaded(tt, hit * 3001) as mx:                                           # every record matches, all in one link cell
        p = _check("one cell", mx, tt, hit * 3001, "chrV", vbin=200, pbin=1000)
        assert p.total == 3001 and p.links == [(4, 0, 0, 3001)] and p.min_loop == 3001 and p.track == [0, 0, 0, 0, 3001]
    every = b"".join(f"r\tchrA\t{1 + i % 5000}\tchrV\t{1 + (i * 7) % 3000}\t+\t-\n".encode() for i in range(5000))
    with _loaded(tt, every) as mx:
        assert _check("everything", mx, tt, every, "chrV", vbin=10, pbin=10).total == 5000
    # whole waves and whole workgroups without a match between matching ones: a match at records 0, 64 * 9 and 256 * 7 + 3 only
    lines = [miss] * 3000
    for at in (0, 64 * 9, 256 * 7 + 3, 2999):
        lines[at] = hit
    sparse = b"".join(lines)
    with _loaded(tt, sparse) as mx:
        assert _check("sparse", mx, tt, sparse, "chrV", vbin=200, pbin=1000).total == 4


@pytest.mark.parametrize("nvb", [LDS_BINS - 1, LDS_BINS, LDS_BINS + 1])
def test_viewpoint_bins_around_the_lds_threshold(nvb):
    """origin 1 and a bin of 1 bp: the viewpoint chromosome has as many bins as bases"""
    _need_gpu()
    table = [("chrA", 5000), ("chrV", nvb)]
    tt = vi.table_text(table)
    rng = random.Random(nvb)
    pos = [1, 2, nvb - 1, nvb] * 3 + [rng.randint(1, nvb) for _ in range(3000)]
    text = "".join(f"r\tchrA\t{rng.randint(1, 5000)}\tchrV\t{p}\t+\t-\n" for p in pos).encode()
    with _loaded(tt, text) as mx:
        p = _check(f"nvb {nvb}", mx, tt, text, "chrV", vbin=1, pbin=100, origin=1)
        assert len(p.track) == nvb and p.track[-1] == 3 + pos[12:].count(nvb) and p.track[0] == 3 + pos[12:].count(1)


@pytest.mark.parametrize("bits,length", [(1, 2), (20, 1 << 20), (32, (1 << 31) + 5)])
def test_key_widths(bits, length):
    """partner bins of 1 bp with origin 1: the table has `length` partner bins and the key holds them in `bits` bits"""
    _need_gpu()
    assert (length - 1).bit_length() == bits
    table = [("chrV", 2000), ("chrP", length)]
    tt = vi.table_text(table)
    rng = random.Random(bits)
    pp = [1, 2, length - 1, length, length, (length + 1) // 2] + [rng.randint(1, length) for _ in range(500)]
    text = "".join(f"r\tchrP\t{max(p, 1)}\tchrV\t{rng.choice([1, 1999, 2000, 77])}\t+\t-\n" for p in pp).encode()
    with _loaded(tt, text) as mx:
        p = _check(f"B {bits}", mx, tt, text, "chrV", vbin=1, pbin=1, origin=1)
        assert max(l[2] for l in p.links) == length - 1 and max(l[0] for l in p.links) == 1999
    if bits == 32:                                                                # 2^32 partner bins or more: refused, with a message
        with m.Matrix(vi.table_text(table + [("chrQ", length)]), [1000000], device=0) as mx:
            mx.add(text)
            mx.run()
            with pytest.raises(m.MktError, match="2\\^32 partner bins"):
                mx.viewpoint("chrV", None, vbin=1, pbin=1, origin=1)
            assert mx.viewpoint("chrV", ["chrP"], vbin=1, pbin=1, origin=1).total == len(pp)


# ---- 3. / 4. the multiset alone decides ---------------------------------------------------------------------------------------------------
def test_order_chunking_route_and_repetition_change_no_byte():
    _need_gpu()
    tt = vi.table_text(SMALL)
    text = _random_text(20000, 5)
    o = dict(vbin=9, pbin=50, hotspot_ratio=0.2, min_count=2)
    lines = text.splitlines(keepends=True)
    random.Random(3).shuffle(lines)
    with _loaded(tt, text) as mx:
        mx.viewpoint("chrV", None, **o)
        whole = _raw(mx)
        mx.viewpoint("chrV", None, **o)
        assert _raw(mx) == whole                                                  # twice
    for other in (dict(pieces=7), dict()):
        with _loaded(tt, text if other else b"".join(lines), **other) as mx:
            mx.viewpoint("chrV", None, **o)
            assert _raw(mx) == whole, other
    swapped = b"".join(b"\t".join([f[0], f[3], f[4], f[1], f[2]] + f[5:]) if not ln.startswith(b"#") else ln for ln in lines for f in [ln.split(b"\t")])
    with _loaded(tt, swapped) as mx:                                              # which side was written first: nothing, when both sides count
        mx.viewpoint("chrV", None, **o)
        assert _raw(mx) == whole


def test_pairs_from_context_keys_give_the_same_bytes():
    _need_gpu()
    import test_gpu_matrix as tm
    tt = tm._table(tm.HG38)
    sam = util.synth("unc", 61, 20000)
    with m.Context("unc", 0.5, 10, False, 4, device=0, block_bytes=1 << 20, ordered=True, extensions=m.EXT_KEYS) as c:
        pairs_text = c.run_bytes(sam, chunk=1 << 20)[0]
        with m.Matrix(tt, [1000000]) as mx:
            mx.add_keys(c, True)
            mx.run()
            # (the context writes the side that is earlier in its order first: chr1 is never the second side, chr9 always is)
            for name, o in (("chr1", dict(vbin=200, pbin=1000000)), ("chr9", dict(vbin=50000, pbin=1000, second_side_only=1, origin=1))):
                got = _check("keys", mx, tt, pairs_text, name, vi.PARTNER_RE, **o)
                assert got.total > 100
                keys = _raw(mx)
                with _loaded(tt, pairs_text) as tx:
                    tx.viewpoint(name, vi.PARTNER_RE, **o)
                    assert _raw(tx) == keys


# ---- 5. state and arguments ------------------------------------------------------------------------------------------------------------------
def test_state_and_arguments():
    _need_gpu()
    tt = vi.table_text(SMALL)
    text = _random_text(3000, 9)
    with m.Matrix(tt, [1000], device=0) as mx:
        mx.add(text)
        with pytest.raises(m.MktError, match="call order violated: viewpoint before run"):
            mx.viewpoint("chrV")
        mx.run()
        with pytest.raises(m.MktError, match="call order violated: no viewpoint profile: viewpoint first"):
            mx._chk(mx.L.mkt_matrix_fetch_viewpoint_track(mx.h, 0, 0, None), "fetch")
        info = mx.viewpoint("chrV", None, vbin=50, pbin=500)
        kept = _raw(mx)
        for bad, msg in ((dict(partners=["chrV", "chrA"]), "its own partner mask"), (dict(vbin=0), "bin size of 0"), (dict(pbin=0), "bin size of 0"), (dict(hotspot_ratio=1.0), r"outside \[0, 1\)"),
                         (dict(hotspot_ratio=1.5), r"outside \[0, 1\)"), (dict(reserved=1), "reserved"), (dict(min_count=0), "min_count"), (dict(origin=2), "origin"), (dict(second_side_only=2), "second_side_only")):
            with pytest.raises(m.MktError, match="bad argument: viewpoint: .*" + msg):
                mx.viewpoint("chrV", bad.pop("partners", None), **bad)
        with pytest.raises(m.MktError, match="viewpoint links"):
            mx._chk(mx.L.mkt_matrix_fetch_viewpoint_links(mx.h, info.links, 1, None, None, None, None), "fetch")
        with pytest.raises(m.MktError, match="viewpoint track bins"):
            mx._chk(mx.L.mkt_matrix_fetch_viewpoint_track(mx.h, info.viewpoint_bins + 1, 0, None), "fetch")
        with pytest.raises(m.MktError, match="viewpoint partner cells"):
            mx._chk(mx.L.mkt_matrix_fetch_viewpoint_partners(mx.h, 0, info.partner_cells_kept + 1, None, None, None), "fetch")
        mx._chk(mx.L.mkt_matrix_fetch_viewpoint_links(mx.h, 0, info.links, None, None, None, None), "fetch")       # any pointer may be NULL
        one = np.zeros(1, np.uint32)
        mx._chk(mx.L.mkt_matrix_fetch_viewpoint_links(mx.h, 3, 1, None, None, None, one.ctypes.data_as(C.c_void_p)), "fetch")
        assert one[0] == mx.viewpoint_result().link_count[3]
        assert _raw(mx) == kept                                                   # every refused call left the results alone
        from microcket_amd.capi import _ViewpointInfoC
        ic = _ViewpointInfoC()
        mx._chk(mx.L.mkt_matrix_viewpoint(mx.h, None, C.byref(ic)), "viewpoint")   # NULL options: the defaults, chromosome 0 against the rest
        names, lens = vd.parse_table(tt)
        assert ic.total == vd.profile(vd.records(text, names, lens), names, 0, {1, 2, 3}).total > 0
        mx.viewpoint("chrV", None, vbin=50, pbin=500)
        assert _raw(mx) == kept
        mx.balance(0, min_nnz=1, mad_max=0)                                        # the analyses of the resolutions leave the profile alone
        assert _raw(mx) == kept
        mx.add(text.splitlines(keepends=True)[-1])                                # add discards
        with pytest.raises(m.MktError, match="viewpoint first|before run"):
            mx._chk(mx.L.mkt_matrix_fetch_viewpoint_track(mx.h, 0, 0, None), "fetch")
        assert mx.viewpoint_timing_ms() == (0.0, 0.0)
        mx.run()
        with pytest.raises(m.MktError, match="viewpoint first"):
            mx._chk(mx.L.mkt_matrix_fetch_viewpoint_track(mx.h, 0, 0, None), "fetch")


def test_executable_without_the_options_is_unchanged_and_checks_its_values(tmp_path):
    _need_gpu()
    (tmp_path / "g.sizes").write_bytes(vi.table_text(SMALL))
    (tmp_path / "in.pairs").write_bytes(_random_text(3000, 21))
    for d in "xy":
        os.makedirs(tmp_path / d)
    run = lambda d, *x: subprocess.run([EXE, "-g", str(tmp_path / "g.sizes"), "-r", "1000,300", "-o", str(tmp_path / d / "o"), "--balance", "--min-nnz", "1", "--mad-max", "0", "--expected", *x,
                                        str(tmp_path / "in.pairs")], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=300)
    runs = [run("x"), run("y", "--viewpoint", "chrV", "--vp-bin", "100")]
    assert all(r.returncode == 0 for r in runs), [r.stderr for r in runs]
    plain = sorted(os.listdir(tmp_path / "x"))
    assert sorted(os.listdir(tmp_path / "y")) == sorted(plain + ["o.viewpoint.bedgraph", "o.viewpoint.links", "o.partners.bedgraph", "o.viewpoint.stat"])
    for f in plain:
        assert open(tmp_path / "x" / f, "rb").read() == open(tmp_path / "y" / f, "rb").read(), f
    stat = dict(ln.split("\t") for ln in open(tmp_path / "y" / "o.viewpoint.stat").read().splitlines())
    assert int(stat["Skipped"]) > 0 and int(stat["Total"]) > 0
    assert run("x", "--vp-bin", "100").returncode == 2                             # a sub-option without --viewpoint or --ebv
    assert run("x", "--vp-second-side").returncode == 2
    for bad in (["--vp-bin", "0"], ["--vp-hotspot", "1"], ["--vp-min-count", "x"], ["--vp-partners", "("], ["--vp-partners", "nothing"], ["--vp-track-bin", "-3"]):
        assert run("x", "--viewpoint", "chrV", *bad).returncode == 12, bad
    assert run("x", "--viewpoint", "chrQ").returncode == 12
    assert run("x", "--ebv").returncode == 12                                      # no chrEBV in this table
    assert sorted(os.listdir(tmp_path / "x")) == plain


# ---- 6. the interface -----------------------------------------------------------------------------------------------------------------------
def test_symbols_and_abi_version():
    _need_gpu()
    L = m.load_library()
    for s in ("mkt_viewpoint_opts_default", "mkt_matrix_viewpoint", "mkt_matrix_fetch_viewpoint_links", "mkt_matrix_fetch_viewpoint_track", "mkt_matrix_fetch_viewpoint_partners",
              "mkt_matrix_viewpoint_timing"):
        assert hasattr(L, s), s
    assert L.mkt_abi_version() == 9
    from microcket_amd.capi import ViewpointOpts
    o = ViewpointOpts()
    L.mkt_viewpoint_opts_default(C.byref(o))
    assert (o.vbin, o.pbin, o.origin, o.second_side_only, o.min_count, o.hotspot_ratio, o.partner_mask) == (200, 1000000, 0, 0, 1, 0.01, None)
