"""The order of the .pairs sorter, restated in Python: what the header comment of mkt_sort.hip states, i.e. what
LANG=C sort -k2,2d -k4,4d -k3,3n -k5,5n gives on pairs text (tab separated, no blanks inside a field):
lines by (chr1 in dictionary order, chr2 in dictionary order, pos1, pos2, whole line bytewise).
tests/test_sortdef_host.py proves it equal to the system's sort; the GPU tests use it where GNU sort is too slow and to explain
a mismatch."""

_DICT = bytes(c for c in range(256) if (48 <= c <= 57) or (65 <= c <= 90) or (97 <= c <= 122) or c in (32, 9))
_DROP = bytes(c for c in range(256) if c not in _DICT)


def dict_form(name: bytes) -> bytes:
    """What -d compares: ASCII alphanumerics and blanks only (LANG=C: bytes)."""
    return name.translate(None, _DROP)


def _num(field: bytes) -> int:
    return int(field) if field else 0                 # sort -n: an empty field counts as 0; leading zeros change nothing


def key(line: bytes):
    """line: one .pairs line without its newline.  Tab is the only field separator."""
    f = line.split(b"\t")
    return (dict_form(f[1]), dict_form(f[3]), _num(f[2]), _num(f[4]), line)


def lines_of(data: bytes):
    lines = data.split(b"\n")
    if lines and lines[-1] == b"":
        lines.pop()
    return lines


def sort_pairs(data: bytes) -> bytes:
    lines = lines_of(data)
    lines.sort(key=key)
    return b"".join(l + b"\n" for l in lines)


def _short(k):
    return tuple(x if not isinstance(x, bytes) or len(x) <= 80 else x[:40] + b"...[%d bytes]..." % len(x) + x[-30:] for x in k)


def explain(got: bytes, want: bytes) -> str:
    """For an assertion message: the first line at which two sorted texts differ, with both keys."""
    if got == want:
        return "equal"
    g, w = lines_of(got), lines_of(want)
    for i in range(min(len(g), len(w))):
        if g[i] != w[i]:
            def k(l):
                try:
                    return _short(key(l))
                except (IndexError, ValueError):
                    return ("not a pairs line", l[:120])
            return f"first difference at line {i} of {len(g)} (want {len(w)}): got key {k(g[i])}, want key {k(w[i])}"
    return f"{len(g)} lines, want {len(w)}; the common part is equal; bytes {len(got)} vs {len(want)}"
