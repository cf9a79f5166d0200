"""The inputs of test_gpu_matrix_edges.py without a GPU: the restated rules of mkt_matrix.hip against values worked out by hand,
the searches over the name table, and what the definition says about every case (the assertions live in the builders of
matrix_edge_cases.py, so that the GPU tests cannot run a case that has drifted off its step)."""
import pytest

import matrix_edge_cases as ec
import matrixdef as md


def test_restated_rules_against_hand_values():
    # FNV-1a 64: the published test vectors of the empty string, "a" and "foobar"
    assert ec.mx_fnv(b"") == 0xcbf29ce484222325 and ec.mx_fnv(b"a") == 0xaf63dc4c8601ec8c and ec.mx_fnv(b"foobar") == 0x85944171f73967e8
    assert ec.home_slot(b"a") == (0xaf63dc4c8601ec8c >> 17) % 16384
    # B: the bits of nbins; the passes: one per started 7-bit digit of 2B bits
    assert [ec.key_bits(n) for n in (1, 2, 3, 4, 127, 128, (1 << 31), (1 << 32) - 1)] == [1, 2, 2, 3, 7, 8, 32, 32]
    assert ec.radix_shifts(7) == [0, 7] and ec.radix_shifts(8) == [0, 7, 14] and ec.radix_shifts(32) == list(range(0, 64, 7)) and ec.radix_shifts(32)[-1] == 63
    assert ec.cell_key(5, 2, 7) == (2 << 3) | 5 and ec.unbinned_key(7) == 0b111111 and ec.unbinned_key(8) == (8 << 4) | 8
    # the k of the issue put 2B below, at and above whole digits
    rem = {(2 * ec.key_bits(n)) % ec.DS_D for k in ec.KEY_WIDTH_K for n in ec.key_width_nbins(k)}
    assert {ec.DS_D - 1, 0, 1} <= rem
    assert len([n for k in ec.KEY_WIDTH_K for n in ec.key_width_nbins(k)]) == 2 * len(ec.KEY_WIDTH_K) - 1
    # a table by hand: two names with one home, the second moves on; a name at the last slot's neighbour wraps
    slots = ec.build_slots([b"a", b"a2"])
    assert slots[ec.home_slot(b"a")] == 0 and ec.probe(slots, [b"a", b"a2"], b"a2")[0] == 1 and ec.probe(slots, [b"a", b"a2"], b"")[0] == -1
    assert ec.probe(slots, [b"a", b"a2"], b"x" * 64) == (-1, [])
    assert ec.run_lengths(1) == [1] and ec.run_lengths(2049) == [1] * 2047 + [2] and sum(ec.run_lengths(16385)) == 16385
    assert ec.run_lengths(8193)[2047:] == [5, 2044, 4096, 1]


@pytest.mark.parametrize("k", ec.KEY_WIDTH_K)
def test_key_width_inputs(k):
    for nbins in ec.key_width_nbins(k):
        case = ec.key_width_case(nbins)
        assert case.facts["B"] == (k if nbins == (1 << k) - 1 else k + 1)


def test_many_resolutions_input():
    ec.many_resolutions_case()


@pytest.mark.parametrize("nv", ec.TILE_NV)
def test_tile_inputs(nv):
    for extra in ec.TILE_EXTRA:
        for shape in ec.TILE_SHAPES:
            case = ec.tile_case(nv, extra, shape)
            assert case.facts == {"n": nv + extra, "nv": nv} and case.text.count(b"\n") == nv + extra
    assert {(ec.TILE_NV.index(v) + s) % 6 for v in ec.TILE_NV for s in range(3)} == set(range(6))   # the single extra line: both kinds, all places


def test_text_nnz_inputs():
    for nnz in ec.TEXT_NNZ:
        ec.text_nnz_case(nnz)


def test_name_table_search():
    nc = ec.name_table_case()
    assert len(nc.names) == ec.K_CHR_SLOTS and len(nc.wrapped) >= 4 and nc.chain[0] >= ec.K_MX_SLOTS - 2 and 0 in nc.chain
    assert nc.chain[:ec.K_MX_SLOTS - nc.chain[0]] == list(range(nc.chain[0], ec.K_MX_SLOTS)) and nc.chain[ec.K_MX_SLOTS - nc.chain[0]] == 0
    # the definition on names: a strict prefix and an extension of a table name are other names
    got = md.definition(b"chr1\t10\nchr10\t10\n", [10], b"r\tchr1\t1\tchr10\t1\nr\tchr\t1\tchr1\t1\nr\tchr100\t1\tchr1\t1\nr\t\t1\tchr1\t1\n")
    assert got[10][0].tolist() == [[0, 1, 1]] and got[10][1] == 3


@pytest.mark.parametrize("which", sorted(ec.POSITION_TABLES))
def test_position_inputs(which):
    ec.positions_case(which)


def test_line_shape_inputs():
    case = ec.line_shapes_case()
    pieces = ec.chunkings(case.text)
    assert set(pieces) == {"whole", "on", "before", "after", "sharp", "bytes"}
    twin = case.text.replace(b"\n", b"\r\n")
    with pytest.raises(ValueError):                                         # a five-column CRLF line: pos2 ends in '\r'
        md.definition(case.table, case.res, twin)
    seven = b"".join(l + b"\n" for l in case.text.split(b"\n") if l.startswith(b"#") or len(l.split(b"\t")) >= 7)
    a, b = md.definition(case.table, case.res, seven), md.definition(case.table, case.res, seven.replace(b"\n", b"\r\n"))
    assert all((a[r][0] == b[r][0]).all() and a[r][1] == b[r][1] for r in case.res) and a[100][0].shape[0] > 5


def test_coo_digit_input():
    case, starts = ec.coo_digits_case()
    assert len(starts) == ec.COO_GROUPS + 1 and case.want[1][0].shape[0] > ec.COO_GROUPS * ec.MX_CPW


def test_partial_table_rule():
    rows, halved, gone = ec.partial_table([(b"a", 100), (b"b", 100), (b"c", 100), (b"d", 100)], b"r\ta\t1\ta\t2\nr\ta\t1\tb\t2\nr\tb\t1\tc\t2\nr\tc\t1\td\t1\n#x\n")
    assert (halved, gone) == (b"a", {b"b", b"c"}) and rows == [(b"a", 50), (b"d", 100)]
