"""The directed cases of tests/paircmp_edge_cases.py without a GPU.
 * Every case reaches the edge it is named for; this is worked out from the texts (offsets in the joined text, positions among the
   data lines, lengths of the lines of the inconsistent text), not taken from the generator.
 * The definition (tests/paircmpdef.py) gives the bytes of tests/golden/paircmp_edges_golden.json, which the reference's script
   printed, for every golden case, and the side and line of every refused case.
 * The stand-alone host program (tests/host/paircmp_host.cpp), plain and sanitized, gives the definition's classes and report for
   every accepted case however the ids are dealt to runs.
 * Seven deliberately wrong variants of the definition -- the mistakes the kernels could make at these edges -- each disagree with
   the definition on at least one new case.  `python tests/test_paircmp_edges_host.py` prints which cases catch which variant, and
   whether the families of paircmp_inputs.CASE_PARAMS would have."""
import hashlib
import json
import operator
import os
import subprocess
import sys

import pytest

import paircmp_edge_cases as ec
import paircmp_inputs as pi
import paircmpdef as pd
import util

HOST = os.path.join(util.ROOT, "tests", "host", "_build", "paircmp_host")
HOST_SAN = HOST + "_san"
GOLDEN = os.path.join(util.GOLDEN, "paircmp_edges_golden.json")
_cache = {}


def sha(b):
    return hashlib.sha256(b).hexdigest()


def want(c):
    """the definition's result of an accepted case, made once"""
    if c["name"] not in _cache:
        _cache[c["name"]] = pd.compare(c["a"], c["b"], int(c["dist"] or 0))
    return _cache[c["name"]]


def golden():
    if "golden" not in _cache:
        with open(GOLDEN) as f:
            _cache["golden"] = {g["name"]: g for g in json.load(f)["cases"]}
    return _cache["golden"]


def layout(c):
    """[(side 0/1, line number from 1, offset of the line in the joined text, the line)]: A, then B, each closed by a newline"""
    out, at = [], 0
    for s in (0, 1):
        for k, r in enumerate(pd.split_lines(c[("a", "b")[s]])):
            out.append((s, k + 1, at, r))
            at += len(r) + 1
    return out


def field_offsets(r):
    out, at = [], 0
    for f in r.split(b"\t")[:5]:
        out.append((at, len(f)))
        at += len(f) + 1
    return out


def is_data(r):
    return not r.startswith(b"#")


def family(name):
    return [c for c in ec.cases() if c["family"] == name]


# ---- the cases sit where they say ---------------------------------------------------------------------------------------------------
def test_case_list_has_every_family_and_the_fields_of_a_case():
    assert {c["family"] for c in ec.cases()} == {"names", "ids_words", "run_at_block_edge", "line_counts", "emit_lengths", "key_widths", "refused", "max_dist"}
    names = [c["name"] for c in ec.cases()]
    assert len(set(names)) == len(names)
    for c in ec.cases():
        assert set(c) >= {"name", "family", "a", "b", "dist", "hash_bits", "golden", "refused"} and isinstance(c["a"], bytes) and isinstance(c["b"], bytes)
        assert max(len(pd.split_lines(c["a"])), len(pd.split_lines(c["b"]))) <= 3100
        assert not (c["golden"] and c["refused"])
    assert [c["name"] for c in ec.cases() if c["golden"]] == list(golden())
    assert ec.cases() is ec.cases() and ec.by_name("names")["a"] is ec.cases()[0]["a"]
    again = ec._build()
    assert [(c["a"], c["b"]) for c in again] == [(c["a"], c["b"]) for c in ec.cases()]          # deterministic


def _name_roles():
    """{role: [(X, Y, offset of X, offset of Y, the bytes behind X, the bytes behind Y, class of the B line)]} of the names case; the
    role is the first letter of the id"""
    c = ec.by_name("names")
    res = want(c)
    rec = {}
    for s, k, at, r in layout(c):
        rec.setdefault(r.split(b"\t")[0], {})[s] = (at, r, k)
    roles = {"c": [], "s": [], "w": []}
    for rid, sides in rec.items():
        if rid.startswith(b"#"):
            continue
        (at_a, ra, ka), (at_b, rb, kb) = sides[0], sides[1]
        oa, ob = field_offsets(ra), field_offsets(rb)
        cls = res.classes_b[kb - 1]
        role = chr(rid[0])
        if role == "c":
            x, y, seen = (at_a, ra, oa[1]), (at_a, ra, oa[3]), cls
        elif role == "s":
            x, y, seen = (at_a, ra, oa[1]), (at_b, rb, ob[1]), cls
        else:
            x, y, seen = (at_a, ra, oa[1]), (at_b, rb, ob[3]), cls
        item = []
        for at, r, (off, n) in (x, y):
            item.append((r[off:off + n], at + off, r[off + n:off + n + 2]))
        roles[role].append((item[0][0], item[1][0], item[0][1], item[1][1], item[0][2], item[1][2], seen, ra, rb))
    return roles


def test_names_meet_every_pair_of_alignments_in_every_role():
    roles = _name_roles()
    expected_diffs = {(n, p) for n in ec.NAME_LENGTHS for p in (0, 6, 7, 8, n - 1) if 0 <= p < n}
    for role, items in roles.items():
        assert len(items) == len(ec.name_pairings()) * ec.NAME_REPS
        compared = [it for it in items if len(it[0]) == len(it[1]) > 0]              # the bytes are compared only at equal lengths
        assert {(it[2] % 8, it[3] % 8) for it in compared} == {(u, v) for u in range(8) for v in range(8)}, role
        by_pair = {}
        for it in compared:
            by_pair.setdefault((it[0], it[1]), []).append(it)
        for (x, y), its in by_pair.items():                                          # every pairing: every alignment of either operand
            assert {it[2] % 8 for it in its} == set(range(8)) and {it[3] % 8 for it in its} == set(range(8)), (role, x, y)
        diffs = set()
        for x, y in by_pair:
            at = [k for k in range(len(x)) if x[k] != y[k]]
            assert len(at) <= 1
            diffs |= {(len(x), k) for k in at}
        assert diffs == expected_diffs, role
        assert {len(it[0]) for it in items if it[0] == it[1]} == set(ec.NAME_LENGTHS), role      # every length with itself, the empty name too
        assert any((it[0], it[1]) == ec.PREFIX_PAIR for it in items) and any((it[1], it[0]) == ec.PREFIX_PAIR for it in items)
        for it in items:
            assert it[4][:1] == b"\t" and it[5][:1] == b"\t"                           # a tab stands behind every name ...
            if role in "sw" and it[0] == it[1]:
                assert it[4][1:] != it[5][1:], (role, it[0])                           # ... and behind equal names other digits
    for it in roles["s"] + roles["w"]:                                                 # only the names decide
        assert it[6] == (pd.CONSISTENT if it[0] == it[1] else pd.DISCORDANT)
    # the same names the other way decide nothing: the second names are equal and the other test fails on its positions
    for it in roles["s"]:
        fa, fb = it[7].split(b"\t"), it[8].split(b"\t")
        assert fa[3] == fb[3] and abs(int(fa[2]) - int(fb[2])) < ec.D and abs(int(fa[2]) - int(fb[4])) >= ec.D
    for it in roles["w"]:
        fa, fb = it[7].split(b"\t"), it[8].split(b"\t")
        assert fa[3] == fb[1] and abs(int(fa[2]) - int(fb[4])) < ec.D and abs(int(fa[4]) - int(fb[2])) < ec.D and abs(int(fa[2]) - int(fb[2])) >= ec.D
    # the role inside one line: the class follows the names, a cis line at every edge of the distribution and the digits behind differ
    gaps = set()
    for it in roles["c"]:
        f = it[7].split(b"\t")
        if it[0] == it[1]:
            gaps.add(abs(int(f[4]) - int(f[2])))
    assert gaps == {0, 999, 1000, 10000, 10001}
    d = want(ec.by_name("names")).info["dist"][0]
    cis = sum(it[0] == it[1] for it in roles["c"])
    assert d["cis_lt_1k"] + d["cis_1_10k"] + d["cis_gt_10k"] == cis and all(d[k] > 0 for k in pd.DIST_KEYS)
    assert any(it[0] == it[1] and it[4][1:] != it[5][1:] for it in roles["c"])


def test_ids_have_the_lengths_and_differ_at_the_word_edges():
    c = ec.by_name("ids_words")
    ids = {r.split(b"\t")[0] for _, _, _, r in layout(c)}
    assert {len(x) for x in ids} == set(ec.ID_LENGTHS) and b"" in ids
    for n in ec.ID_LENGTHS:
        same = sorted(x for x in ids if len(x) == n)
        base = ec.ALPHA[:n]
        diffs = {k for x in same for k in range(n) if x[k] != base[k]}
        assert base in same and diffs == {p for p in (0, 7, 8, n - 1) if 0 <= p < n}, n
        assert all(sum(x[k] != base[k] for k in range(n)) <= 1 for x in same)
    res = want(c)
    assert all(res.info[k] >= 5 for k in ("consistent", "discordant", "a_only", "b_only"))
    assert c["hash_bits"] == [0, 1, 2] and len(ids) > 4                                # narrowed: several ids share every run


def test_value_and_claimant_lie_on_both_sides_of_a_workgroup_edge():
    cases = family("run_at_block_edge")
    assert sorted((c["shape"], c["k"]) for c in cases) == sorted((s, k) for s in ("a_long", "comments", "b_long") for k in ec.EDGE_KS)
    assert {k % ec.SWG for k in ec.EDGE_KS} == {ec.SWG - 1, 0, 1} and len({k // ec.SWG for k in ec.EDGE_KS}) == 3
    verdicts = set()
    for c in cases:
        rows = layout(c)
        data = [(s, k, r) for s, k, _, r in rows if is_data(r)]                         # one id: this is the sorted order at every width
        assert {r.split(b"\t")[0] for _, _, r in data} == {b"h"} and c["hash_bits"] == [0, 5]
        value = max(j for j, (s, _, _) in enumerate(data) if s == 0)
        claimant = min(j for j, (s, _, _) in enumerate(data) if s == 1)
        k = c["k"]
        if c["shape"] == "b_long":
            assert (value, claimant) == (0, 1) and len(data) == k + 1                  # the B-only lines cross the edges
        else:
            assert (value, claimant) == (k - 1, k) and len(data) == k + 2
        res = want(c)
        a, b = data[value], data[claimant]
        gap = abs(int(a[2].split(b"\t")[2]) - int(b[2].split(b"\t")[2]))
        assert gap == (ec.D - 1 if k % 2 == 0 else ec.D)
        cls = res.classes_b[b[1] - 1]
        assert cls == res.classes_a[a[1] - 1] == (pd.CONSISTENT if k % 2 == 0 else pd.DISCORDANT)
        verdicts.add((c["shape"], cls))
        assert res.info["consistent"] + res.info["discordant"] == 1 and res.info["a_only"] == 0
        assert res.classes_a.count(pd.SUPERSEDED) == (0 if c["shape"] == "b_long" else k - 1)
        assert res.info["b_only"] == (k - 1 if c["shape"] == "b_long" else 1)
        comments = [sum(not is_data(r) for s, _, _, r in rows if s == side) for side in (0, 1)]
        assert all(n > 1 for n in comments) if c["shape"] == "comments" else comments == [0, 0]
        if c["shape"] == "comments":                                                   # interleaved: comments before, between and behind
            for side in (0, 1):
                kinds = [is_data(r) for s, _, _, r in rows if s == side]
                assert not kinds[0] and not kinds[-1] and True in kinds[1:-1] and False in kinds[1:-1]
    assert verdicts == {(s, v) for s in ("a_long", "comments", "b_long") for v in (pd.CONSISTENT, pd.DISCORDANT)}


def test_line_counts_are_the_listed_ones():
    seen = set()
    for c in family("line_counts"):
        info = want(c).info
        if c["total"] is not None:
            assert sum(info["lines"]) == c["total"] and info["data_lines"] == info["lines"]
            seen.add((c["total"], info["lines"][0]))
    assert seen == {(n, k) for n in ec.COUNT_TOTALS for k in (0, n, 1, 128)}
    info = {c["name"]: want(c).info for c in family("line_counts")}
    assert info["comments_both"]["lines"] == [3, 3] and info["comments_both"]["data_lines"] == [0, 0]
    assert info["comments_a_data_b"]["data_lines"] == [0, 5] and info["comments_a_data_b"]["lines"][0] == 3
    assert info["data_a_comments_b"]["data_lines"] == [5, 0] and info["data_a_comments_b"]["lines"][1] == 3
    c = ec.by_name("empty_a_b_unterminated")
    assert c["a"] == b"" and not c["b"].endswith(b"\n") and info[c["name"]]["lines"] == [0, 5]
    c = ec.by_name("a_unterminated_empty_b")
    assert c["b"] == b"" and not c["a"].endswith(b"\n") and info[c["name"]]["lines"] == [5, 0]
    c = ec.by_name("one_hash")
    assert (c["a"], c["b"]) == (b"#", b"") and info["one_hash"]["lines"] == [1, 0] and info["one_hash"]["data_lines"] == [0, 0]


def test_emitted_lines_have_the_listed_lengths():
    c = ec.by_name("emit_lengths")
    res = want(c)
    rows = res.lines.split(b"\n")[:-1]
    length = {kind: {len(r) + 1 for r in rows if r[:1] == kind} for kind in (b"A", b"B", b"I")}
    assert length[b"A"] >= set(ec.EMIT_LENGTHS) and length[b"B"] >= set(ec.EMIT_LENGTHS)
    assert length[b"I"] >= {n for n in ec.EMIT_LENGTHS if n >= ec.EMIT_I_MIN}
    assert ec.EMIT_I_MIN == len(b"I\t" + b"\t" + b"\t1\t\t2" + b"\tvs\t" + b"\t1\t\t2" + b"\n")          # empty id, empty names, one digit
    parts = [set(), set(), set()]                                                      # the id and its tab, A's four fields, B's four fields
    for r in rows:
        if r[:1] == b"I":
            f = r.split(b"\t")
            assert len(f) == 11 and f[6] == b"vs"
            for k, n in enumerate((len(f[1]) + 1, len(b"\t".join(f[2:6])), len(b"\t".join(f[7:11])))):
                parts[k].add(n)
    assert all(p >= set(ec.EMIT_PARTS) for p in parts)
    src = [{r.split(b"\t")[0]: r for r in pd.split_lines(c[s])} for s in ("a", "b")]
    counts = {(src[0][r.split(b"\t")[1]].count(b"\t") + 1, src[1][r.split(b"\t")[1]].count(b"\t") + 1) for r in rows if r[:1] == b"I"}
    assert {(5, 12), (12, 5)} <= counts
    ends = {(src[0][r.split(b"\t")[1]].endswith(b"\t"), src[1][r.split(b"\t")[1]].endswith(b"\t")) for r in rows if r[:1] == b"I"}
    assert {(True, False), (False, True)} <= ends                                      # the fifth field before a newline here, a tab there
    kinds = b"".join(r[:1] for r in rows)
    ib = kinds.rstrip(b"A")
    assert b"A" not in ib and kinds[len(ib):] and ib.count(b"IB") >= 9 and ib.count(b"BI") >= 9     # B's order, then A's lines
    b_ids = [r.split(b"\t")[0] for r in pd.split_lines(c["b"])]
    assert [r.split(b"\t")[1] for r in rows[:len(ib)]] == [x for x in b_ids if res.classes_b[b_ids.index(x)] in (pd.ONLY, pd.DISCORDANT)]
    assert res.info["consistent"] >= 2 and res.info["discordant"] >= 20
    for name, head in (("empty_id_a_only", b"A\t\tc\t"), ("empty_id_b_only", b"B\t\tc\t"), ("empty_id_discordant", b"I\t\tc\t")):
        assert any(r.startswith(head) for r in want(ec.by_name(name)).lines.split(b"\n")), name


def test_every_case_with_several_claimed_pairs_has_both_verdicts():
    single = []
    for c in ec.accepted():
        info = want(c).info
        if info["consistent"] + info["discordant"] >= 2:
            assert info["consistent"] and info["discordant"], c["name"]
        elif info["consistent"] + info["discordant"] == 1:
            single.append(c["name"])
    # one claimed pair cannot have both: the single-id texts, one line in A, the empty id in both files next to one other id
    assert all(n.startswith(("edge_", "count_", "empty_id_")) for n in single)
    for fam in ("names", "ids_words", "run_at_block_edge", "line_counts", "emit_lengths", "key_widths", "max_dist"):
        tot = [sum(want(c).info[k] for c in family(fam)) for k in ("consistent", "discordant")]
        assert all(tot), fam


def test_key_width_cases_hold_more_ids_than_narrow_keys():
    cases = {c["name"]: c for c in family("key_widths")}
    assert all(c["hash_bits"] == [2, 5, 13, 31, 32] for c in cases.values())
    for name, gen in (("repeats", dict(kind="repeats", seed=5)), ("lines", dict(kind="lines", seed=12))):
        assert (cases["widths_" + name]["a"], cases["widths_" + name]["b"]) == pi.make(gen)
        assert gen == next(p["gen"] for p in pi.CASE_PARAMS if p["name"] == name)
    c = cases["widths_mixed_3000"]
    assert 3000 <= len(pd.split_lines(c["a"])) <= 3100
    ids = {r.split(b"\t")[0] for _, _, _, r in layout(c) if is_data(r)}
    assert len(ids) > (1 << 5) and len({r.split(b"\t")[0] for _, _, _, r in layout(cases["widths_repeats"])}) > (1 << 2)
    assert {(w + 3) // 4 * 4 for w in ec.KEY_WIDTHS} == {4, 8, 16, 32} and {w % 4 for w in ec.KEY_WIDTHS} >= {0, 1, 2, 3}


# ---- the definition: golden bytes and refusals -------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", [c["name"] for c in ec.cases() if c["golden"]])
def test_definition_gives_the_reference_bytes(name):
    c, g = ec.by_name(name), golden()[name]
    res = want(c)
    assert g["dist"] == c["dist"]
    assert pd.report(res, "{A}", "{B}").decode() == g["stdout"]
    assert (res.lines_ib.count(b"\n"), res.lines_a.count(b"\n")) == (g["lines_ib"], g["lines_a"])
    assert sha(res.lines_ib) == g["sha256_ib"]
    assert sha(b"".join(sorted(res.lines_a.splitlines(keepends=True)))) == g["sha256_a_sorted"]


def _all_bad(c):
    """every line of a case that alone would be refused, as (side, line number, index in the joined numbering)"""
    out = []
    na = len(pd.split_lines(c["a"]))
    for s, k, _, r in layout(c):
        try:
            pd.parse(r + b"\n", "AB"[s])
        except pd.BadLine:
            out.append(("AB"[s], k, k - 1 + (na if s else 0)))
    return out


@pytest.mark.parametrize("name", [c["name"] for c in ec.refused()])
def test_definition_refuses_by_side_and_line(name):
    c = ec.by_name(name)
    with pytest.raises(pd.BadLine) as e:
        pd.compare(c["a"], c["b"])
    assert (e.value.side, e.value.number) == c["refused"]
    bad = _all_bad(c)
    assert (bad[0][0], bad[0][1]) == c["refused"]                                      # the smallest in the joined numbering


def test_refused_cases_put_their_bad_lines_where_they_say():
    bad = {c["name"][len("refused_"):]: _all_bad(c) for c in ec.refused()}
    for name in ("two_in_b", "two_in_a", "a600_b3", "both_workgroups_of_b"):
        assert len(bad[name]) == 2 and len({j // ec.SWG for _, _, j in bad[name]}) == 2, name       # two workgroups of the parse
    assert {s for s, _, _ in bad["a600_b3"]} == {"A", "B"} and bad["a600_b3"][1][1] < bad["a600_b3"][0][1]
    assert [bad[f"joined_{j}"] for j in (255, 256, 257)] == [[("A", 256, 255)], [("B", 1, 256)], [("B", 2, 257)]]
    rows = {c["name"][len("refused_"):]: layout(c)[bad[c["name"][len("refused_"):]][0][2]][3] for c in ec.refused()}
    f = {k: r.split(b"\t") for k, r in rows.items()}
    assert f["pos_20_digits"][2] == b"9" * 20 and f["pos_small_mod_2_32"][4] == b"4294967301" and int(f["pos_small_mod_2_32"][4]) % (1 << 32) == 5
    assert (f["pos_plus"][2], f["pos_minus"][4], f["pos_blank_first"][2], f["pos_blank_last"][4]) == (b"+5", b"-5", b" 5", b"5 ")
    assert rows["cr_behind_the_fifth_field"].endswith(b"\t5\r") and rows["four_tabs_only"] == b"\t" * 4 and rows["tabs_2000"] == b"\t" * 2000
    assert rows["empty_fifth_field"].count(b"\t") == 4 and rows["empty_fifth_field"].endswith(b"\t") and all(f["empty_fifth_field"][:4])
    for c in ec.refused():                                                             # accepted apart from what is listed
        drop = {(x, y) for x, y, _ in bad[c["name"][len("refused_"):]]}
        keep = [[r for k, r in enumerate(pd.split_lines(c[s])) if (s.upper(), k + 1) not in drop] for s in ("a", "b")]
        pd.compare(ec.text(keep[0]), ec.text(keep[1]))


def test_max_dist_cases_are_the_names_text_at_the_top_of_the_type():
    names = ec.by_name("names")
    assert [c["dist"] for c in family("max_dist")] == [str(1 << 31), str((1 << 32) - 1)]
    for c in family("max_dist"):
        assert (c["a"], c["b"]) == (names["a"], names["b"]) and not c["golden"]
        assert want(c).max_dist == int(c["dist"]) and want(c).info["discordant"] > 0 and want(c).info["consistent"] > 0


# ---- the host half of the library ------------------------------------------------------------------------------------------------------
def _host(exe, tmp_path, c, bits):
    fa, fb = tmp_path / "a.pairs", tmp_path / "b.pairs"
    fa.write_bytes(c["a"])
    fb.write_bytes(c["b"])
    return subprocess.run([exe, str(fa), str(fb), c["dist"] or "0", str(bits), "{A}", "{B}"], stdout=subprocess.PIPE, stderr=subprocess.PIPE)


@pytest.mark.parametrize("bits", [0, 2, 5])
@pytest.mark.parametrize("san", [False, True], ids=["plain", "sanitized"])
def test_host_half_gives_the_classes_and_the_report(san, bits, tmp_path):
    util.ensure_built()
    exe = HOST_SAN if san else HOST
    assert os.path.exists(exe), exe
    for c in ec.accepted():
        r = _host(exe, tmp_path, c, bits)
        assert r.returncode == 0, (c["name"], r.returncode, r.stderr.decode()[-2000:])
        la, ca, lb, cb, rep = r.stdout.split(b"\n", 4)
        res = want(c)
        assert la == b"classes A %d" % len(ca) and lb == b"classes B %d" % len(cb), c["name"]
        assert bytes(x - 48 for x in ca) == res.classes_a and bytes(x - 48 for x in cb) == res.classes_b, c["name"]
        assert rep == pd.report(res, "{A}", "{B}"), c["name"]
        if c["golden"]:
            assert rep.decode() == golden()[c["name"]]["stdout"], c["name"]


def test_host_driver_refuses_by_side_and_line(tmp_path):
    util.ensure_built()
    for c in ec.refused():
        r = _host(HOST_SAN, tmp_path, c, 2)
        assert r.returncode == 3 and b"file %s line %d " % (c["refused"][0].encode(), c["refused"][1]) in r.stderr, (c["name"], r.stderr)


# ---- wrong variants of the definition: what the cases are there to catch ---------------------------------------------------------------
def _exact(r, off, n, what):
    return r[off:off + n]


def _decimal(x):
    return int(x) if x.isdigit() and x.isascii() and int(x) < (1 << 31) else None


def restated(a, b, max_dist, key=_exact, pos=_decimal, near=operator.lt, pick=min, blind=None):
    """The definition once more with its parts open to change: key(line, offset, length, "id" or "name") is what two strings are
    compared by, pos(text) a position or None, near(d, D) the bound, pick which of the refused (side, line) is reported.  blind: None
    joins by id as the definition does; False / True join every record from its two neighbours among the data lines as k_pc_join
    does (texts with ONE id only, where that order is A's lines, then B's), with True a record at a multiple of 256 not seeing the
    one before it.  -> ("refused", side, line) or ("ok", classes A, classes B, dist, I/B lines, A lines)"""
    D = max_dist or 200
    sides, bad = [], []
    for s, t in enumerate((a, b)):
        recs = []
        for k, r in enumerate(pd.split_lines(t)):
            rec = None
            if not r.startswith(b"#"):
                f = r.split(b"\t")
                p = [pos(x) for x in (f[2], f[4])] if len(f) >= 5 else [None]
                if None in p:
                    bad.append((s, k + 1))
                else:
                    o = field_offsets(r)
                    rec = dict(f=tuple(f[:5]), id=key(r, *o[0], "id"), c1=key(r, *o[1], "name"), c2=key(r, *o[3], "name"), p1=p[0], p2=p[1])
            recs.append(rec)
        sides.append(recs)
    if bad:
        s, k = pick(bad)
        return ("refused", "AB"[s], k)

    def consistent(x, y):
        return (x["c1"] == y["c1"] and near(abs(x["p1"] - y["p1"]), D) and x["c2"] == y["c2"] and near(abs(x["p2"] - y["p2"]), D)) or \
               (x["c1"] == y["c2"] and near(abs(x["p1"] - y["p2"]), D) and x["c2"] == y["c1"] and near(abs(x["p2"] - y["p1"]), D))

    ra, rb = sides
    ca, cb = bytearray(len(ra)), bytearray(len(rb))
    dist = [[0] * 4, [0] * 4]
    for s in (0, 1):
        for r in sides[s]:
            if r is not None:
                d = abs(r["p2"] - r["p1"])
                dist[s][3 if r["c1"] != r["c2"] else 2 if d > 10000 else 0 if d < 1000 else 1] += 1
    partner = {}
    if blind is None:
        value = {}
        for k, r in enumerate(ra):
            if r is not None:
                if r["id"] in value:
                    ca[value[r["id"]]] = pd.SUPERSEDED
                value[r["id"]] = k
                ca[k] = pd.ONLY
        for k, r in enumerate(rb):
            if r is not None:
                cb[k] = pd.ONLY
                if r["id"] in value:
                    j = partner[k] = value.pop(r["id"])
                    ca[j] = cb[k] = pd.CONSISTENT if consistent(ra[j], r) else pd.DISCORDANT
    else:
        data = [(0, k) for k, r in enumerate(ra) if r is not None] + [(1, k) for k, r in enumerate(rb) if r is not None]
        assert len({sides[s][k]["id"] for s, k in data}) <= 1
        for j, (s, k) in enumerate(data):
            prev = data[j - 1] if j > 0 and not (blind and j % ec.SWG == 0) else None
            nxt = data[j + 1] if j + 1 < len(data) else None
            if s == 0:
                ca[k] = pd.ONLY if nxt is None else pd.SUPERSEDED if nxt[0] == 0 else pd.CONSISTENT if consistent(ra[k], rb[nxt[1]]) else pd.DISCORDANT
            elif prev is not None and prev[0] == 0:
                cb[k] = pd.CONSISTENT if consistent(ra[prev[1]], rb[k]) else pd.DISCORDANT
                partner[k] = prev[1]
            else:
                cb[k] = pd.ONLY
    ib = []
    for k, r in enumerate(rb):
        if cb[k] == pd.ONLY:
            ib.append(b"\t".join((b"B",) + r["f"]) + b"\n")
        elif cb[k] == pd.DISCORDANT:
            ib.append(b"\t".join((b"I", r["f"][0]) + ra[partner[k]]["f"][1:] + (b"vs",) + r["f"][1:]) + b"\n")
    al = [b"\t".join((b"A",) + r["f"]) + b"\n" for k, r in enumerate(ra) if ca[k] == pd.ONLY]
    return ("ok", bytes(ca), bytes(cb), dist, b"".join(ib), b"".join(al))


def defined(a, b, max_dist):
    try:
        res = pd.compare(a, b, max_dist)
    except pd.BadLine as e:
        return ("refused", e.side, e.number)
    return ("ok", res.classes_a, res.classes_b, [[d[k] for k in pd.DIST_KEYS] for d in res.info["dist"]], res.lines_ib, res.lines_a)


def _single_id(a, b):
    try:
        return len({r[0] for t in (a, b) for r in pd.parse(t, "A") if r is not None}) == 1
    except pd.BadLine:
        return False


VARIANTS = {
    "a: names equal when their first 8 bytes are": dict(key=lambda r, off, n, what: (n, r[off:off + min(n, 8)]) if what == "name" else r[off:off + n]),
    "b: the last n % 8 bytes ignored when n >= 8": dict(key=lambda r, off, n, what: (n, r[off:off + (n - n % 8 if n >= 8 else n)])),
    # a tab stands behind every id and every name, in both operands, so one byte more decides nothing in this format; two do
    "c: the bytes behind the strings compared too": dict(key=lambda r, off, n, what: (n, r[off:off + n + 2])),
    "d: no predecessor at multiples of 256": dict(blind=True),
    "e: positions modulo 2^32": dict(pos=lambda x: int(x) % (1 << 32) if x.isdigit() and x.isascii() and int(x) % (1 << 32) < (1 << 31) else None),
    "f: the largest refused line reported": dict(pick=max),
    "g: <= D in place of < D": dict(near=operator.le),
}


def caught_by(variant, texts):
    """the names of the (name, a, b, max_dist) on which a variant disagrees with the definition"""
    out = []
    for name, a, b, D in texts:
        kw = VARIANTS[variant]
        if "blind" in kw and not _single_id(a, b):
            continue                                                                   # the sorted order is known for one id only
        if restated(a, b, D, **kw) != defined(a, b, D):
            out.append(name)
    return out


def new_texts():
    return [(c["name"], c["a"], c["b"], int(c["dist"] or 0)) for c in ec.cases()]


def old_texts():
    if "old" not in _cache:
        _cache["old"] = [(p["name"],) + pi.make(p["gen"]) + (int(p["dist"] or 0),) for p in pi.CASE_PARAMS]
    return _cache["old"]


def test_restatement_with_nothing_changed_is_the_definition():
    for name, a, b, D in new_texts() + old_texts():
        assert restated(a, b, D) == defined(a, b, D), name
        if _single_id(a, b):
            assert restated(a, b, D, blind=False) == defined(a, b, D), name


@pytest.mark.parametrize("variant", list(VARIANTS))
def test_every_wrong_variant_is_caught_by_a_new_case(variant):
    got = caught_by(variant, new_texts())
    print(variant, "->", got[:6], len(got))
    assert got, variant
    expect = {"a": "names", "b": "names", "c": "names", "d": "edge_a_long_256", "e": "refused_pos_small_mod_2_32", "f": "refused_two_in_b", "g": "edge_a_long_255"}
    assert expect[variant[0]] in got


def table():
    rows = ["| variant | new cases that catch it | families of CASE_PARAMS that catch it |", "|---|---|---|"]
    for v in VARIANTS:
        new, old = caught_by(v, new_texts()), caught_by(v, old_texts())
        fams = sorted({ec.by_name(n)["family"] for n in new})
        rows.append(f"| {v} | {len(new)} ({', '.join(fams)}) | {', '.join(old) if old else 'none'} |")
    return "\n".join(rows)


if __name__ == "__main__":
    sys.stdout.write(table() + "\n")
