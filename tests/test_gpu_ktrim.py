"""Adapter and quality trimming on the GPU: mkt_trim_* (through microcket_amd.Trimmer / trim) against the golden vectors made by
Ktrim 1.6.0 (tests/golden/ktrim_golden.json) and the definition (tests/ktrimdef.py), byte for byte, by every route."""
import pytest

import ktrim_cases as kc
import ktrimdef as kd
import microcket_amd as m
from test_ktrim_def import batch_input, batch_output, case_input, golden

pytestmark = pytest.mark.gpu


def _need_gpu():
    if m.device_count() < 1:
        pytest.fail("no HIP device")


def split_of(il):
    """the two split files of an interleaved stream"""
    return kd.split_interleaved(il)


def test_seeded_goldens_by_hash():
    _need_gpu()
    with m.Trimmer() as t:
        for c in golden()["cases"]:
            t1, t2 = case_input(c)
            t.begin(**c["opts"]).push(t1, t2, final=True)
            assert kd.sha(t.interleaved()) == c["stdout_sha256"], c["name"]
            assert (kd.sha(t.read1()), kd.sha(t.read2())) == (c["read1_sha256"], c["read2_sha256"]), c["name"]
            assert t.log_text() == c["log"], c["name"]
            st = t.stats()
            assert st.total == c["pairs"] and st.total == st.dropped + st.passed, c["name"]


def test_directed_goldens():
    _need_gpu()
    with m.Trimmer() as t:
        for b in golden()["batches"]:
            t1, t2 = batch_input(b)
            t.begin(**b["opts"]).push(t1, t2, final=True)
            want = batch_output(b)
            assert t.interleaved() == want, b["name"]
            assert (t.read1(), t.read2()) == split_of(want), b["name"]
            assert t.log_text() == b["log"], b["name"]


@pytest.mark.parametrize("segment_pairs", [1, 7, 1 << 20])
def test_segment_size_does_not_change_the_bytes(segment_pairs):
    _need_gpu()
    b = next(x for x in golden()["batches"] if x["name"] == "length_grid")
    t1, t2 = batch_input(b)
    with m.Trimmer(segment_pairs=segment_pairs) as t:
        t.begin().push(t1, t2, final=True)
        assert t.interleaved() == batch_output(b) and t.log_text() == b["log"]
    c = golden()["cases"][0]
    t1, t2 = case_input(c)
    if segment_pairs > 1:
        with m.Trimmer(segment_pairs=segment_pairs) as t:
            half = len(t1) // 2
            t.begin().push(t1[:half], t2[:half + 1000]).push(t1[half:], t2[half + 1000:], final=True)
            assert kd.sha(t.interleaved()) == c["stdout_sha256"] and t.log_text() == c["log"]


def _six():
    """six short pairs: untouched, adapter, tail hit, dropped by quality, dimer, untouched"""
    rec = [kc.pair("a", 90, 44, seed=1), kc.pair("b", 37, 44, seed=2), kc.pair("c", 42, 44, seed=3), kc.pair("d", 90, 44, q1="I" * 20 + "#" * 24, seed=4),
           kc.pair("e", 1, 44, seed=5), kc.pair("f", 90, 40, L2=38, seed=6)]
    t1, t2 = kc.text_of(rec)
    return t1, t2, kd.trim_stream(t1, t2)


def test_pushes_split_at_every_byte():
    _need_gpu()
    t1, t2, (il, r1, r2, st) = _six()
    assert st[0] == 6 and 0 < st[5]
    with m.Trimmer(segment_pairs=2) as t:
        for cut in range(len(t1) + 1):      # both streams cut at the same offset
            t.begin().push(t1[:cut], t2[:cut]).push(t1[cut:], t2[cut:], final=True)
            assert (t.interleaved(), t.read1(), t.read2()) == (il, r1, r2), cut
        for cut in range(0, len(t1) + 1, 7):      # unequal pieces: read 1 runs ahead, read 2 comes late
            t.begin().push(t1[:cut], b"").push(t1[cut:], t2[:cut // 3]).push(b"", t2[cut // 3:], final=True)
            assert (t.interleaved(), t.read1(), t.read2()) == (il, r1, r2), cut
        assert tuple(t.stats()) == st


def test_missing_final_newline():
    _need_gpu()
    t1, t2, (il, r1, r2, st) = _six()
    assert m.trim(t1[:-1], t2[:-1])[:3] == (il, r1, r2)


def test_interleaved_input_equals_two_streams():
    _need_gpu()
    c = golden()["cases"][1]
    t1, t2 = case_input(c)
    a, b = kd.parse(t1), kd.parse(t2)
    text = b"".join(b"%s\n%s\n+\n%s\n%s\n%s\n+\n%s\n" % (x + y) for x, y in zip(a, b))
    with m.Trimmer(segment_pairs=500) as t:
        t.begin(interleaved_input=True, **c["opts"])
        for k in range(0, len(text), 99991):
            t.push(text[k:k + 99991])
        t.push(final=True)
        assert kd.sha(t.interleaved()) == c["stdout_sha256"] and t.log_text() == c["log"]


def test_second_run_on_one_object():
    _need_gpu()
    c = golden()["cases"][3]
    t1, t2 = case_input(c)
    with m.Trimmer() as t:
        first = t.begin(**c["opts"]).push(t1, t2, final=True).interleaved()
        assert kd.sha(first) == c["stdout_sha256"]
        assert t.begin(**c["opts"]).push(t1, t2, final=True).interleaved() == first and t.log_text() == c["log"]
        assert all(x >= 0 for x in t.timing_ms()) and sum(t.timing_ms()) > 0


@pytest.mark.parametrize("name", [r[0] for r in kc.REFUSED_INPUT])
def test_refused_input(name):
    _need_gpu()
    _, t1, t2, opts, what = next(r for r in kc.REFUSED_INPUT if r[0] == name)
    with pytest.raises(ValueError):
        kd.trim_stream(t1, t2, **opts)
    with m.Trimmer() as t:
        with pytest.raises(m.MktError, match=what):
            t.begin(**opts).push(t1, t2, final=True)
        good1, good2, (il, _, _, _) = _six()      # the object serves the next run
        assert t.begin().push(good1, good2, final=True).interleaved() == il


def test_refused_options_and_states():
    _need_gpu()
    with m.Trimmer() as t:
        for name, opts, _ in kc.REFUSED_OPTIONS:
            with pytest.raises(m.MktError):
                t.begin(**opts)
        with pytest.raises(m.MktError):
            t.begin(interleaved_input=True).push(b"@a\n", b"@b\n")
    with pytest.raises(m.MktError):
        m.Trimmer(segment_pairs=0)
    with m.Trimmer() as t:
        with pytest.raises(m.MktError):
            t.push(b"", b"", final=True)      # before begin
