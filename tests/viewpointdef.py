"""The viewpoint contact profile of include/mkt.h (mkt_matrix_viewpoint) restated in plain Python, from the .pairs text and the
chromosome table alone: the matching rule, the two binnings, the link table, the two tracks, the hotspot cut and the three texts.
With origin 0 and second_side_only 1 the texts are those of the reference's util/analyze.EBV scripts (tests/golden/
viewpoint_golden.json holds what the scripts wrote)."""
import collections
import math
import re

Profile = collections.namedtuple("Profile", "total links track partners partner_cells min_loop links_kept")


def parse_table(ttext):
    names, lens = [], []
    for ln in ttext.decode().split("\n"):
        ln = ln.rstrip("\r")
        if ln and not ln.startswith("#"):
            f = ln.split("\t")
            names.append(f[0])
            lens.append(int(f[1]))
    return names, lens


def records(text, names, lens):
    """(ia, pa, ib, pb) of every pair the matrix stage accepts, sides as written: '#' lines are no pairs; a pair with a chromosome
    outside the table or a position of 0 or past the length is skipped"""
    index = {n: i for i, n in enumerate(names)}
    out = []
    for ln in text.decode().split("\n"):
        if not ln or ln.startswith("#"):
            continue
        f = ln.split("\t")
        a, b = index.get(f[1]), index.get(f[3])
        pa, pb = int(f[2]), int(f[4])
        if a is None or b is None or not (1 <= pa <= lens[a]) or not (1 <= pb <= lens[b]):
            continue
        out.append((a, pa, b, pb))
    return out


def partner_set(names, viewpoint, partners):
    """None: every other chromosome; a string: a regular expression applied with re.search; else a list of names"""
    if partners is None:
        return {i for i in range(len(names)) if i != viewpoint}
    if isinstance(partners, str):
        return {i for i, n in enumerate(names) if re.search(partners, n)}
    return {names.index(n) for n in partners}


def min_loop_of(counts, total, ratio):
    """the hotspot cut from the link counts"""
    if not counts:
        return 0
    hist = collections.Counter(counts)
    cutoff = int(total * ratio)
    largest = max(hist)
    min_loop = largest + 1
    accum = 0
    for v in sorted(hist, reverse=True):
        accum += v * hist[v]
        if accum > cutoff:
            min_loop = v + 1
            break
    return min(min_loop, largest)


def profile(recs, names, viewpoint, partners, vbin=200, pbin=1000000, origin=0, second_side_only=0, min_count=1, hotspot_ratio=0.01):
    """recs: (ia, pa, ib, pb); viewpoint: a table index; partners: a set of table indices without the viewpoint"""
    assert viewpoint not in partners
    link = collections.Counter()
    vt = collections.Counter()
    pt = collections.Counter()
    total = 0
    for ia, pa, ib, pb in recs:
        if ia in partners and ib == viewpoint:
            pc, pp, vp = ia, pa, pb
        elif ia == viewpoint and ib in partners and not second_side_only:
            pc, pp, vp = ib, pb, pa
        else:
            continue
        i, j = (vp - origin) // vbin, (pp - origin) // pbin
        link[(i, pc, j)] += 1
        vt[i] += 1
        pt[(pc, j)] += 1
        total += 1
    links = [k + (link[k],) for k in sorted(link)]
    track = [vt[i] for i in range(max(vt) + 1)] if vt else []
    cells = sorted(pt, key=lambda k: (names[k[0]].encode(), k[1]))
    part = [k + (pt[k],) for k in cells if pt[k] >= min_count]
    ml = min_loop_of([l[3] for l in links], total, hotspot_ratio)
    return Profile(total, links, track, part, len(cells), ml, sum(1 for l in links if l[3] >= ml))


def hs_name(name):
    return name.replace("chr", "hs", 1)


def track_text(p, name, vbin):
    return "".join(f"{name}\t{i * vbin}\t{i * vbin + vbin}\t{c}\n" for i, c in enumerate(p.track)).encode()


def partners_text(p, names, pbin):
    return "".join(f"{names[c]}\t{j * pbin}\t{j * pbin + pbin}\t{k}\n" for c, j, k in p.partners).encode()


def links_text(p, names, vbin, pbin):
    keyed = sorted((f"{i}\t{hs_name(names[c])}\t{j}".encode(), i, c, j, k) for i, c, j, k in p.links if k >= p.min_loop)
    out = []
    for _, i, c, j, k in keyed:
        t = int(math.log(float(k)) / math.log(2.0))
        out.append(f"hs0\t{i * vbin * 5000}\t{i * vbin * 5000 + vbin * 5000}\t{hs_name(names[c])}\t{j * pbin}\t{j * pbin + pbin}\tthickness={t}p\n")
    return "".join(out).encode()


def ebv_texts(text, ttext, viewpoint_name, partner_re, vbin, pbin, ratio, track_bin, min_count):
    """the three texts of the reference's analysis (the rule of its scripts: origin 0, the viewpoint on the second side)"""
    names, lens = parse_table(ttext)
    recs = records(text, names, lens)
    v = names.index(viewpoint_name)
    ps = partner_set(names, v, partner_re) - {v}
    a = profile(recs, names, v, ps, vbin=vbin, pbin=pbin, origin=0, second_side_only=1, hotspot_ratio=ratio)
    b = profile(recs, names, v, ps, vbin=vbin, pbin=track_bin, origin=0, second_side_only=1, min_count=min_count, hotspot_ratio=ratio)
    return track_text(a, viewpoint_name, vbin), links_text(a, names, vbin, pbin), partners_text(b, names, track_bin)
