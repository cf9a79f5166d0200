"""The lean tile path at its parser, window and capacity edges, on the CPU: every case of tests/fast_edge_cases.py through the
oracle and through the emulation of the tile phases (tests/host/tile_emul.cpp: the generic path alone, and the lean path with the
generic one behind it, both in the 48 KiB geometry the GPU test forces).  Outputs byte for byte, and the number of tiles the
lean path took against what the case declares: a case that quietly went to the generic path fails here, so the GPU test
(test_gpu_fast_edges.py), which asks the kernel for the same number, is about k_fast."""
import pytest

import fast_edge_cases as ec
import util

PARAMS = ((4, 0.5, 10, True), (2, 0.8, 0, False))
NAMES = [c[0] for c in ec.cases()]


@pytest.mark.parametrize("name", NAMES)
def test_case_against_oracle_and_reference(name):
    _, text, modes, expect = ec.case(name)
    for mode in modes:
        for (T, ratio, mapq, sam) in PARAMS:
            tag = (name, mode, T, ratio, mapq, sam)
            po, so, lo, st = util.oracle_run(text, mode, T, ratio, mapq, sam)
            for cfg in (0, 10):
                pe, se, le, es = util.emul_run(text, mode, T, ratio, mapq, sam, cfg, 0)
                assert es["err"] == 0, tag + (cfg,)
                assert pe == po and se == so and le == lo, tag + (cfg,)      # (the emulation keeps input order)
                assert es["groups"] == st.groups, tag + (cfg,)
            assert es["tiles"] == ec.ntiles(text) and es["blocks"] == 1, tag
            assert es["lean_tiles"] == (es["tiles"] if expect == "all" else expect), tag + (es["lean_tiles"], es["tiles"])
            if util.have_ref() and name not in ec.REF_UNPINNED:
                rc, rp, rs, rl, err = util.ref_run(text, mode, T, ratio, mapq, sam)
                assert rc == 0, tag + (err,)
                assert util.canon(rp) == util.canon(po) and util.canon(rs) == util.canon(so) and rl == lo, tag


@pytest.mark.parametrize("block", ec.BLOCK_SIZES)
@pytest.mark.parametrize("name", ec.MULTIBLOCK)
def test_several_blocks(name, block):
    """the same text cut into blocks of 4 KiB and of a tile and three lines: windows at a block's start and end many times over"""
    _, text, modes, _ = ec.case(name)
    for mode in modes:
        for (T, ratio, mapq, sam) in PARAMS:
            po, so, lo, st = util.oracle_run(text, mode, T, ratio, mapq, sam)
            for cfg in (0, 10):
                pe, se, le, es = util.emul_run(text, mode, T, ratio, mapq, sam, cfg, block)
                assert es["err"] == 0 and es["blocks"] > 1, (name, mode, cfg, block)
                assert pe == po and se == so and le == lo and es["groups"] == st.groups, (name, mode, cfg, block)


def test_every_boundary_has_both_sides():
    """what the case module promises: no case is "either", refused cases lose exactly one tile, and each limit has its two sides"""
    by = {c[0]: c for c in ec.cases()}
    for name, text, modes, expect in ec.cases():
        assert expect == "all" or (isinstance(expect, int) and expect == ec.ntiles(text) - 1), name
        assert set(modes) <= set(ec.BOTH) and modes, name
        assert text.endswith(b"\n") or "no_newline" in name, name
    pairs = [("qname_5", "qname_4"), ("qname_62", "qname_63"), ("sep6_rname_64", "sep6_rname_65"), ("sep6_cigar_64", "sep6_cigar_65"),
             ("flag_forms", "flag_11_chars"), ("pos_forms", "pos_11_chars"), ("mapq_forms", "mapq_11_chars"), ("cigar_forms", "cigar_33_bytes"),
             ("cigar_forms", "cigar_count_10_digits"), ("window_of_168_lines", "window_of_169_lines"), ("short_line_two_vectors", "short_line_one_vector"),
             ("group_of_63", "group_of_64"), ("last_group_of_64", "last_group_of_65"), ("group_to_halo_line_11", "group_to_halo_line_12"),
             ("prev_survivor_63_back_new_name", "prev_survivor_64_back_new_name"), ("prev_survivor_62_back_same_name", "prev_survivor_63_back_same_name"),
             ("first_survivor_is_line_63", "first_survivor_is_line_64"), ("flash_96_reporting_groups", "flash_97_reporting_groups")]
    pairs += [("head_soff%d_last" % s, "head_soff%d_past" % s) for s in (0, 1, 8, 16)]
    pairs += [("text_length_%02d" % r, "text_length_%02d_no_newline" % r) for r in range(16)]
    for lean, refused in pairs:
        assert by[lean][3] == "all" and by[refused][3] != "all", (lean, refused)
    assert ec.window_lines(by["window_of_168_lines"][1])[1] == ec.LCAP and ec.window_lines(by["window_of_169_lines"][1])[1] == ec.LCAP + 1


def test_chr_cache_names_collide():
    """the counters case of the GPU test: more short names than fast_chr_slot's 64-entry cache holds, crowded into few two-way sets"""
    names = [n for n in ec.chr_cache_names() if len(n) <= 6]
    assert len(names) == 70 and len(set(names)) == 70 and {len(n) for n in names} >= {1, 2, 3, 4}
    sets = {}
    for n in names:
        sets.setdefault(ec.cc_idx(n) >> 1, []).append(n)
    assert max(len(v) for v in sets.values()) >= 5 and len(sets) <= 24, sorted((len(v) for v in sets.values()), reverse=True)
    assert sum(1 for n in ec.chr_cache_names() if len(n) >= 7) >= 3
