// pairs2matrix -- the computation behind the driver's last stage (microcket:520-554: `juicer_tools pre -r 2500000,...,5000` and
// `cooler cload pairix GINFO:minBIN`) on the GPU: final.pairs -> the sparse binned contact matrix at every resolution asked for.
// The .hic / .cool containers themselves are not written; the output is what `cooler load -f coo <chrom.sizes>:<r>` ingests.
// The work is mkt_matrix_* of libmkt_hip.so (include/mkt.h, where the binning is defined); this file only moves bytes.
//
//   pairs2matrix -g <chrom.sizes> -r r1[,r2,...] -o <prefix> [in.pairs ...]        (no input file: stdin; $MKT_DEVICE: GPU ordinal)
//                [--balance [--ignore-diags N] [--min-nnz N] [--min-count N] [--mad-max X] [--tol X] [--max-iters N]] [--expected]
//                [--loops [--loop-peak N] [--loop-window N] [--loop-window-max N] [--loop-min-ll-count N] [--loop-min-dist N]
//                         [--loop-max-dist N] [--loop-fdr X] [--loop-cluster-radius N]]
//                [--eigs [--eigs-n N] [--eigs-ignore-diags N] [--eigs-clip X] [--eigs-min-good N] [--eigs-tol X] [--eigs-max-iters N]
//                        [--eigs-track FILE]]
//                [--insulation BP1[,BP2,..] [--ins-ignore-diags N] [--ins-min-frac-valid X] [--ins-min-strength X]]
//                [--apa] [--pileup FILE.bedpe] [--pile-flank N] [--pile-corner N] [--pile-kind balanced|oe|oe-smooth] [--pile-edges]
//                [--saddle [--saddle-groups N] [--saddle-trim LO,HI] [--saddle-contact cis|trans] [--saddle-kind oe|oe-smooth]
//                          [--saddle-min-dist BP] [--saddle-max-dist BP] [--saddle-corner N]]
//                [--compare OTHER.pairs [--scc-h N] [--scc-min-dist BP] [--scc-max-dist BP] [--scc-weighting n|var]]
//                [--viewpoint NAME | --ebv] [--vp-bin BP] [--vp-partner-bin BP] [--vp-track-bin BP] [--vp-min-count N] [--vp-hotspot R]
//                                           [--vp-partners REGEX] [--vp-second-side]
//
// Writes per resolution <prefix>.<r>.coo (lines bin1 \t bin2 \t count, made on the device; empty for an empty matrix) and
// <prefix>.<r>.bins.bed (chrom \t start \t end per bin, end clipped to the chromosome length), and <prefix>.matrix.stat
// (Pairs, Binned, Skipped, then nnz.<r> per resolution).
// With --balance (iterative correction, mkt_matrix_balance of include/mkt.h) also per resolution <prefix>.<r>.weights.bed (the lines of
// .bins.bed with a fourth column: the bin's weight as %.17g, nan for a masked bin) and <prefix>.balance.stat (per resolution
// r, iterations, converged 0/1, var, scale, masked bins); a resolution that did not converge is a warning.  Without --balance nothing
// of this is written and every other byte is the same.  A sub-option without --balance is a usage error, a malformed value exit 12.
// With --expected (mkt_matrix_expected of include/mkt.h; with --balance from the weights, without it raw: every bin valid, weight 1)
// also per resolution, each with a header line, doubles as %.17g and nan for NaN:
//   <prefix>.<r>.expected.tsv         diag, dist_bp = diag * r, n_valid, count_sum, balanced_sum, expected, expected_smooth (genome-wide)
//   <prefix>.<r>.expected.chrom.tsv   chrom, diag, n_valid, count_sum, balanced_sum (every diagonal of every chromosome)
//   <prefix>.<r>.expected.trans.tsv   chrom1, chrom2, n_valid, count_sum, balanced_sum, expected (every pair in table order)
// Without --expected none of these appears and every other byte is the same.  A per-cell text dump of balanced or observed / expected
// values is out of scope (mkt_matrix_fetch_values hands them back as arrays).
// With --loops (mkt_matrix_loops of include/mkt.h; it implies --expected and, like it, uses the weights with --balance and raw counts
// without) also per resolution <prefix>.<r>.loops.bedpe: a header line, then per loop in the order of the library chrom, start, end of
// the peak's two bins, count, the four raw expected values (donut, ll, h, v; %.17g), window, cells of the component and its bounding box
// (start1, end1, start2, end2); and <prefix>.loops.stat (per resolution r, cells, candidates, tested, undefined, over, grew, at_max,
// enriched, loops).  Without --loops neither appears and every other byte is the same.  A sub-option without --loops is a usage error, a
// malformed value or a window outside peak < window <= window-max <= 20 exit 12, before anything is read.
// With --eigs (mkt_matrix_eigs of include/mkt.h: compartment eigenvectors; it implies --expected and, like it, uses the weights with
// --balance and raw counts without) also per resolution <prefix>.<r>.eigs.tsv: a header line, then the columns of .bins.bed plus E1 .. Ek
// as %.17g (nan for NaN); and <prefix>.eigs.stat, one row per resolution and chromosome: r, chrom, bins, good, iterations, converged,
// lambda1 .. lambdak.  A chromosome that did not converge is a warning.  --eigs-track FILE: a four-column bed with exactly the bins of
// .bins.bed in order whose fourth column (a number or nan) fixes the sign; only with a single resolution (a usage error otherwise), a row
// that does not match is exit 12.  Without --eigs neither file appears and every other byte is the same.  A sub-option without --eigs is
// a usage error, a malformed value exit 12.
// With --insulation BP1[,BP2,..] (mkt_matrix_insulation of include/mkt.h: diamond insulation scores and boundaries; 1 .. 4 window sizes in
// base pairs, strictly ascending, each a positive multiple of every -r and at most 1024 bins, otherwise exit 12 before anything is read;
// from the weights with --balance, raw counts without) also per resolution <prefix>.<r>.insulation.tsv: a header line, then the columns
// of .bins.bed plus per window n_valid_<bp>, score_<bp>, log2_insulation_score_<bp>, boundary_strength_<bp> (doubles as %.17g, nan for
// NaN) and is_boundary_<bp> (0 / 1); and <prefix>.insulation.stat, one row per resolution and window: r, window_bp, bins, defined,
// minima, boundaries.  Without --insulation neither appears and every other byte is the same.  A sub-option without --insulation is a
// usage error, a malformed value exit 12.
// With --apa (mkt_matrix_pileup of include/mkt.h around the peak cells of the loops, in loop order: aggregate peak analysis; it implies
// --loops and with it --expected) also per resolution <prefix>.<r>.apa.tsv: a header line, then side^2 rows p, q, n, csum, vsum, mean in
// ascending (p, q), doubles as %.17g and nan for NaN; and <prefix>.apa.stat, one row per resolution: r, features, used, trans, edge, dist,
// peak, p2ll, p2ul, p2ur, p2lr, p2m, z_ll.  With --pileup FILE.bedpe (it implies --expected) the same around the pairs of anchors of the
// file as <prefix>.<r>.pileup.tsv and <prefix>.pileup.stat: six tab-separated columns or more (chrom1, start1, end1, chrom2, start2,
// end2), '#' lines and empty lines skipped; an anchor's bin is that of its midpoint (start + end) / 2, a pair whose first bin is the
// larger is swapped; an unknown chromosome, a midpoint at or past the chromosome's length or a malformed line is exit 12 before anything
// is read.  --pile-flank (1 .. 32, default 10), --pile-corner (1 .. flank, default 6, or the flank when that is smaller), --pile-kind
// (default oe-smooth) and --pile-edges (clip the windows of features near a chromosome's end instead of leaving those features out) hold
// for both; one of them without --apa or --pileup is a usage error, a bad value exit 12.  Without the two flags none of these files
// appears and every other byte is the same.
// With --saddle (mkt_matrix_saddle of include/mkt.h with eigenvector 1 as the track, oriented by --eigs-track when that is given; it
// implies --eigs) also per resolution <prefix>.<r>.saddle.tsv: a header line, then one row per pair of groups a <= b: a, b, n, nnz, csum,
// vsum, mean, doubles as %.17g and nan for NaN; and <prefix>.saddle.stat, per resolution one "info" row (r, info, n_groups, candidates,
// kept, cells_used, chunks, corner, strength, aa_ab, bb_ab), one "group" row per group (r, group, g, bins, lo, hi) and one "profile" row
// per k = 1 .. n_groups / 2 (r, profile, k, strength, aa_ab, bb_ab).  --saddle-groups (2 .. 64, default 50), --saddle-trim LO,HI (basis
// points, default 250,250), --saddle-contact (default cis), --saddle-kind (default oe), --saddle-min-dist / --saddle-max-dist (base pairs,
// each a multiple of every -r; defaults: diagonals 2 and up, no upper limit), --saddle-corner (1 .. groups / 2; default max(1, groups / 5)).
// One of them without --saddle is a usage error, a bad value exit 12.  Without --saddle neither file appears and every other byte is the
// same.
// With --compare OTHER.pairs (mkt_matrix_scc of include/mkt.h: the stratum-adjusted correlation of the input and a replicate) the second
// file is binned with the same table and resolutions; with --balance both matrices are balanced with the same options and the weights
// are used, without it raw counts.  Also per resolution <prefix>.<r>.scc.tsv: a header line, then the strata table, one row per
// chromosome and diagonal: chrom, diag, dist_bp, n_cand, n, sx, sy, sxx, syy, sxy, rho, w, doubles as %.17g and nan for NaN; and
// <prefix>.scc.stat, per resolution one "chrom" row per chromosome (r, chrom, name, scored strata, num, den, scc) and one "genome" row
// (r, genome, n_chrom, strata, candidates, used, scored, count_a, count_b, scc).  --scc-h (0 .. 16, default 5), --scc-min-dist (default
// 0) and --scc-max-dist (default 5000000, rounded down to whole bins and at least one bin; 0 = every diagonal) in base pairs, each given
// value a multiple of every -r, --scc-weighting (default n).  One of them without --compare is a usage error, a bad value exit 12.
// Without --compare neither file appears and every other byte is the same.
// With --viewpoint NAME (mkt_matrix_viewpoint of include/mkt.h: the contacts of one chromosome with the rest of the genome, the
// reference's util/analyze.EBV) also <prefix>.viewpoint.bedgraph (NAME, start, end, count for the viewpoint bins 0 .. the last occupied
// one, bins of --vp-bin, default 200), <prefix>.viewpoint.links (Circos links of the cells above the hotspot cut of --vp-hotspot, default
// 0.01, partner bins of --vp-partner-bin, default 1000000), <prefix>.partners.bedgraph (a second profile with partner bins of
// --vp-track-bin, default 1000: the cells with at least --vp-min-count pairs, default 1, by name and start) and <prefix>.viewpoint.stat.
// --vp-partners REGEX keeps the chromosomes whose name the expression finds (ECMAScript, unanchored; default: every other chromosome);
// --vp-second-side counts only pairs whose second side is on the viewpoint.  --ebv is the preset of the reference's analyze.EBV.sh:
// --viewpoint chrEBV --vp-partners 'chr\d+$' --vp-second-side --vp-min-count 5, the other defaults as above, each --vp-* still
// overriding; for a pairs file the matrix stage accepts in full the first three files are then byte for byte what the reference's
// calc.inter.EBV.matrix.and.circos.pl (stdout, stderr) and calc.loop2EBV.pl | LC_ALL=C sort -k1,1 -k2,2n write.  DEVIATIONS: pairs the
// matrix stage skips (unknown chromosome, position outside the length; "Skipped" of the .stat) are absent here where the Perl counts
// them; without a matching pair the bedgraph is empty where the Perl prints a line of zeros; juicer_tools pre of analyze.EBV.sh is out
// of scope.  One of --vp-* without --viewpoint or --ebv is a usage error, a bad value, an unknown NAME or an expression that keeps
// nothing exit 12.  Without the two flags none of these files appears and every other byte is the same.
// With --hic (mkt_matrix_hic of include/mkt.h) also <prefix>.hic, every resolution in one container (with --balance the weights as
// normalisation vectors of the label --hic-norm-label, default ICE), and <prefix>.hic.stat (file bytes, matrices, blocks, float blocks,
// pieces, raw and deflated bytes, level, block bins).  --hic-level 0 .. 2 (default 2), --hic-block-bins 1 .. 32767 (default 1000),
// --hic-genome ID (default empty).  One of them without --hic is a usage error, a value that is no number exit 12.  Without --hic
// neither file appears and every other byte is the same.
// Exit codes: 0 ok, 2 usage, 10 unreadable input or table, 12 bad table / resolution list, 20 no GPU, 21 library error, 22 write failure.
#include <cerrno>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <regex>
#include <string>
#include <vector>
#include "../../include/mkt.h"
#include "mkt_viewpoint.h"

static int usage(const char* me) {
    fprintf(stderr, "Usage: %s -g <chrom.sizes> -r r1[,r2,...] -o <prefix> [in.pairs ...]\n"
                    "       [--balance [--ignore-diags N] [--min-nnz N] [--min-count N] [--mad-max X] [--tol X] [--max-iters N]] [--expected]\n"
                    "       [--loops [--loop-peak N] [--loop-window N] [--loop-window-max N] [--loop-min-ll-count N] [--loop-min-dist N]\n"
                    "                [--loop-max-dist N] [--loop-fdr X] [--loop-cluster-radius N]]\n"
                    "       [--eigs [--eigs-n N] [--eigs-ignore-diags N] [--eigs-clip X] [--eigs-min-good N] [--eigs-tol X] [--eigs-max-iters N]\n"
                    "               [--eigs-track FILE]]\n"
                    "       [--insulation BP1[,BP2,..] [--ins-ignore-diags N] [--ins-min-frac-valid X] [--ins-min-strength X]]\n"
                    "       [--apa] [--pileup FILE.bedpe] [--pile-flank N] [--pile-corner N] [--pile-kind balanced|oe|oe-smooth] [--pile-edges]\n"
                    "       [--saddle [--saddle-groups N] [--saddle-trim LO,HI] [--saddle-contact cis|trans] [--saddle-kind oe|oe-smooth]\n"
                    "                 [--saddle-min-dist BP] [--saddle-max-dist BP] [--saddle-corner N]]\n"
                    "       [--compare OTHER.pairs [--scc-h N] [--scc-min-dist BP] [--scc-max-dist BP] [--scc-weighting n|var]]\n"
                    "       [--viewpoint NAME | --ebv] [--vp-bin BP] [--vp-partner-bin BP] [--vp-track-bin BP] [--vp-min-count N] [--vp-hotspot R]\n"
                    "                                  [--vp-partners REGEX] [--vp-second-side]\n"
                    "       [--hic [--hic-level N] [--hic-block-bins N] [--hic-genome ID] [--hic-norm-label S]]\n", me);
    return 2;
}
static bool read_file(const char* fn, std::string& out) {
    FILE* f = fopen(fn, "rb");
    if (!f) return false;
    char buf[65536];
    size_t k;
    while ((k = fread(buf, 1, sizeof buf, f)) > 0) out.append(buf, k);
    const bool ok = !ferror(f);
    fclose(f);
    return ok;
}
struct Chrom { std::string name; uint64_t len; };
// name \t length [\t ...] per line; empty and '#' lines ignored (the library checks the same things: this copy gives exit code 12
// before a GPU is asked for, and the bins for the .bed files)
static bool parse_table(const std::string& txt, std::vector<Chrom>& out, std::string& why) {
    size_t p = 0, line = 0;
    while (p < txt.size()) {
        size_t q = txt.find('\n', p);
        if (q == std::string::npos) q = txt.size();
        size_t e = q;
        ++line;
        if (e > p && txt[e - 1] == '\r') --e;
        if (e > p && txt[p] != '#') {
            const size_t t = txt.find('\t', p);
            if (t == std::string::npos || t >= e || t == p || t - p > 63) { why = "line " + std::to_string(line) + ": name<TAB>length needed (name of 1 .. 63 bytes)"; return false; }
            size_t d = t + 1;
            uint64_t v = 0;
            size_t nd = 0;
            while (d < e && txt[d] >= '0' && txt[d] <= '9' && nd < 11) { v = v * 10 + (uint64_t)(txt[d] - '0'); ++d; ++nd; }
            if (nd == 0 || (d < e && txt[d] != '\t') || v > 0xFFFFFFFFull) { why = "line " + std::to_string(line) + ": no length (a decimal number below 2^32)"; return false; }
            for (const Chrom& c : out) if (c.name == txt.substr(p, t - p)) { why = "line " + std::to_string(line) + ": " + c.name + " is there twice"; return false; }
            out.push_back({txt.substr(p, t - p), v});
        }
        p = q + 1;
    }
    if (out.empty()) { why = "no chromosome"; return false; }
    if (out.size() > 8192) { why = "more than 8192 chromosomes"; return false; }
    return true;
}
static bool parse_res(const char* s, std::vector<uint32_t>& out) {
    const char* p = s;
    for (;;) {
        uint64_t v = 0;
        int nd = 0;
        while (*p >= '0' && *p <= '9' && nd < 11) { v = v * 10 + (uint64_t)(*p - '0'); ++p; ++nd; }
        if (nd == 0 || v == 0 || v > 0xFFFFFFFFull) return false;
        for (uint32_t x : out) if (x == v) return false;
        out.push_back((uint32_t)v);
        if (*p == '\0') break;
        if (*p != ',') return false;
        ++p;
    }
    return out.size() <= 16;
}
static bool write_file(const std::string& fn, const char* p, size_t n, const char* mode = "wb") {
    FILE* f = fopen(fn.c_str(), mode);
    if (!f) return false;
    const bool ok = (n == 0 || fwrite(p, 1, n, f) == n);
    return (fclose(f) == 0) && ok;
}

// a whole non-negative decimal integer below 2^31 / a whole non-negative finite number
static bool parse_int(const char* s, int32_t& out) {
    if (!*s) return false;
    uint64_t v = 0;
    for (const char* p = s; *p; ++p) { if (*p < '0' || *p > '9' || p - s >= 10) return false; v = v * 10 + (uint64_t)(*p - '0'); }
    if (v > 0x7FFFFFFFull) return false;
    out = (int32_t)v;
    return true;
}
static bool parse_num(const char* s, double& out) {
    if (!*s || !((*s >= '0' && *s <= '9') || *s == '.')) return false;           // no sign, no inf / nan, no leading blank
    for (const char* p = s; *p; ++p)                                              // plain decimal, with or without an exponent: no hexadecimal float
        if (!((*p >= '0' && *p <= '9') || *p == '.' || *p == 'e' || *p == 'E' || ((*p == '+' || *p == '-') && (p[-1] == 'e' || p[-1] == 'E')))) return false;
    char* end = nullptr;
    errno = 0;
    const double v = strtod(s, &end);
    if (errno || *end || !(v >= 0.0) || v > 1.7976931348623157e308) return false;
    out = v;
    return true;
}

static void put_num(std::string& out, double x) {
    char num[40];
    if (x != x) strcpy(num, "nan"); else snprintf(num, sizeof num, "%.17g", x);
    out += num;
}

// a start or an end of a BEDPE line: a whole non-negative decimal number
static bool parse_coord(const std::string& f, uint64_t& out) {
    if (f.empty() || f.size() > 18) return false;
    uint64_t v = 0;
    for (char ch : f) { if (ch < '0' || ch > '9') return false; v = v * 10 + (uint64_t)(ch - '0'); }
    out = v;
    return true;
}
// chrom1, start1, end1, chrom2, start2, end2 [, ...] per line -> (chromosome index, midpoint) twice per feature
struct Anchor { size_t c1, c2; uint64_t m1, m2; };
static bool parse_bedpe(const std::string& txt, const std::vector<Chrom>& chroms, std::vector<Anchor>& out, std::string& why) {
    size_t p = 0, line = 0;
    while (p < txt.size()) {
        size_t q = txt.find('\n', p);
        if (q == std::string::npos) q = txt.size();
        size_t e = q;
        ++line;
        if (e > p && txt[e - 1] == '\r') --e;
        if (e > p && txt[p] != '#') {
            std::string f[6];
            size_t at = p;
            int k = 0;
            for (; k < 6; ++k) {
                size_t t = at;
                while (t < e && txt[t] != '\t') ++t;
                f[k] = txt.substr(at, t - at);
                if (t >= e) { ++k; break; }
                at = t + 1;
            }
            if (k < 6) { why = "line " + std::to_string(line) + ": six tab-separated columns are needed (chrom1, start1, end1, chrom2, start2, end2)"; return false; }
            Anchor a;
            uint64_t v[4];
            for (int j = 0; j < 4; ++j)
                if (!parse_coord(f[j < 2 ? 1 + j : 2 + j], v[j])) { why = "line " + std::to_string(line) + ": '" + f[j < 2 ? 1 + j : 2 + j] + "' is not a position"; return false; }
            if (v[1] < v[0] || v[3] < v[2]) { why = "line " + std::to_string(line) + ": an end before its start"; return false; }
            for (int side = 0; side < 2; ++side) {
                const std::string& nm = f[side ? 3 : 0];
                size_t c = 0;
                while (c < chroms.size() && chroms[c].name != nm) ++c;
                if (c == chroms.size()) { why = "line " + std::to_string(line) + ": unknown chromosome " + nm; return false; }
                const uint64_t mid = (v[2 * side] + v[2 * side + 1]) / 2;
                if (mid >= chroms[c].len) { why = "line " + std::to_string(line) + ": midpoint " + std::to_string(mid) + " is past the end of " + nm + " (" + std::to_string(chroms[c].len) + ")"; return false; }
                (side ? a.c2 : a.c1) = c; (side ? a.m2 : a.m1) = mid;
            }
            out.push_back(a);
        }
        p = q + 1;
    }
    return true;
}
// the arrays and the info of the last mkt_matrix_pileup of resolution index k as <fn> and one more row of `stat`
static int write_pileup(mkt_matrix* m, uint32_t k, uint32_t r, const mkt_pileup_info& pi, const std::string& fn, std::string& stat) {
    const size_t S = pi.side, S2 = S * S;
    std::vector<uint64_t> n(S2), cs(S2);
    std::vector<double> vs(S2), mean(S2);
    const int rc = mkt_matrix_fetch_pileup(m, k, n.data(), cs.data(), vs.data(), mean.data());
    if (rc != MKT_OK) return rc;
    std::string t = "p\tq\tn\tcsum\tvsum\tmean\n";
    const int flank = (int)(S / 2);
    for (size_t x = 0; x < S2; ++x) {
        t += std::to_string((int)(x / S) - flank); t += '\t'; t += std::to_string((int)(x % S) - flank); t += '\t'; t += std::to_string(n[x]); t += '\t'; t += std::to_string(cs[x]); t += '\t';
        put_num(t, vs[x]); t += '\t'; put_num(t, mean[x]); t += '\n';
    }
    if (!write_file(fn, t.data(), t.size())) return -1;
    stat += std::to_string(r);
    for (uint64_t v : {pi.features, pi.used, pi.trans, pi.edge, pi.dist}) { stat += '\t'; stat += std::to_string(v); }
    for (double v : {pi.peak, pi.p2ll, pi.p2ul, pi.p2ur, pi.p2lr, pi.p2m, pi.z_ll}) { stat += '\t'; put_num(stat, v); }
    stat += '\n';
    return MKT_OK;
}

// the tables, the group edges and the profile of the last mkt_matrix_saddle of resolution index k as <fn> and more rows of `stat`
static int write_saddle(mkt_matrix* m, uint32_t k, uint32_t r, const mkt_saddle_info& si, const std::string& fn, std::string& stat) {
    const size_t Q = si.n_groups, Q2 = Q * Q;
    std::vector<uint64_t> n(Q2), nz(Q2), cs(Q2), gb(Q);
    std::vector<double> vs(Q2), mean(Q2), lo(Q), hi(Q), st(Q / 2), aa(Q / 2), bb(Q / 2);
    int rc = mkt_matrix_fetch_saddle(m, k, n.data(), nz.data(), cs.data(), vs.data(), mean.data());
    if (rc == MKT_OK) rc = mkt_matrix_fetch_saddle_edges(m, k, gb.data(), lo.data(), hi.data());
    if (rc == MKT_OK) rc = mkt_matrix_fetch_saddle_profile(m, k, st.data(), aa.data(), bb.data());
    if (rc != MKT_OK) return rc;
    std::string t = "a\tb\tn\tnnz\tcsum\tvsum\tmean\n";
    for (size_t a = 0; a < Q; ++a)
        for (size_t b = a; b < Q; ++b) {
            const size_t x = a * Q + b;
            t += std::to_string(a); t += '\t'; t += std::to_string(b); t += '\t'; t += std::to_string(n[x]); t += '\t'; t += std::to_string(nz[x]); t += '\t';
            t += std::to_string(cs[x]); t += '\t'; put_num(t, vs[x]); t += '\t'; put_num(t, mean[x]); t += '\n';
        }
    if (!write_file(fn, t.data(), t.size())) return -1;
    const std::string rs = std::to_string(r);
    stat += rs; stat += "\tinfo";
    for (uint64_t v : {(uint64_t)si.n_groups, si.candidates, si.kept, si.cells_used, (uint64_t)si.chunks, (uint64_t)si.corner}) { stat += '\t'; stat += std::to_string(v); }
    for (double v : {si.strength, si.aa_ab, si.bb_ab}) { stat += '\t'; put_num(stat, v); }
    stat += '\n';
    for (size_t g = 0; g < Q; ++g) {
        stat += rs; stat += "\tgroup\t"; stat += std::to_string(g); stat += '\t'; stat += std::to_string(gb[g]); stat += '\t'; put_num(stat, lo[g]); stat += '\t'; put_num(stat, hi[g]); stat += '\n';
    }
    for (size_t j = 0; j < Q / 2; ++j) {
        stat += rs; stat += "\tprofile\t"; stat += std::to_string(j + 1); stat += '\t'; put_num(stat, st[j]); stat += '\t'; put_num(stat, aa[j]); stat += '\t'; put_num(stat, bb[j]); stat += '\n';
    }
    return MKT_OK;
}

// the strata table and the per-chromosome scores of the last mkt_matrix_scc of resolution index k as <fn> and more rows of `stat`
static int write_scc(mkt_matrix* m, uint32_t k, uint32_t r, const mkt_scc_info& ci, int32_t min_diag, const std::vector<Chrom>& chroms, const std::string& fn, std::string& stat) {
    const size_t D = ci.strata, rows = (size_t)ci.n_chrom * D;
    std::vector<uint64_t> nc(rows), nu(rows), sc(ci.n_chrom);
    std::vector<double> v[7], cs(ci.n_chrom), cn(ci.n_chrom), cd(ci.n_chrom);
    for (auto& x : v) x.resize(rows);
    int rc = mkt_matrix_fetch_scc_strata(m, k, 0, rows, nc.data(), nu.data(), v[0].data(), v[1].data(), v[2].data(), v[3].data(), v[4].data(), v[5].data(), v[6].data());
    if (rc == MKT_OK) rc = mkt_matrix_fetch_scc_chrom(m, k, 0, ci.n_chrom, cs.data(), cn.data(), cd.data(), sc.data());
    if (rc != MKT_OK) return rc;
    std::string t = "chrom\tdiag\tdist_bp\tn_cand\tn\tsx\tsy\tsxx\tsyy\tsxy\trho\tw\n";
    const char* md = "wb";
    for (size_t c = 0; c < ci.n_chrom; ++c)
        for (size_t j = 0; j < D; ++j) {
            const size_t at = c * D + j;
            const uint64_t d = (uint64_t)min_diag + j;
            t += chroms[c].name; t += '\t'; t += std::to_string(d); t += '\t'; t += std::to_string(d * r); t += '\t'; t += std::to_string(nc[at]); t += '\t'; t += std::to_string(nu[at]);
            for (auto& x : v) { t += '\t'; put_num(t, x[at]); }
            t += '\n';
            if (t.size() > ((size_t)32 << 20)) { if (!write_file(fn, t.data(), t.size(), md)) return -1; t.clear(); md = "ab"; }
        }
    if (!write_file(fn, t.data(), t.size(), md)) return -1;
    const std::string rs = std::to_string(r);
    for (size_t c = 0; c < ci.n_chrom; ++c) {
        stat += rs; stat += "\tchrom\t"; stat += chroms[c].name; stat += '\t'; stat += std::to_string(sc[c]); stat += '\t'; put_num(stat, cn[c]); stat += '\t'; put_num(stat, cd[c]);
        stat += '\t'; put_num(stat, cs[c]); stat += '\n';
    }
    stat += rs; stat += "\tgenome";
    for (uint64_t x : {(uint64_t)ci.n_chrom, (uint64_t)ci.strata, ci.candidates, ci.used, ci.scored, ci.count_a, ci.count_b}) { stat += '\t'; stat += std::to_string(x); }
    stat += '\t'; put_num(stat, ci.scc); stat += '\n';
    return MKT_OK;
}

int main(int argc, char* argv[]) {
    const char *table = nullptr, *rlist = nullptr, *prefix = nullptr;
    std::vector<const char*> files;
    bool balance = false, expected = false, loops = false, eigs = false;
    const char* gopt[7] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
    static const char* const gname[7] = {"--eigs-n", "--eigs-ignore-diags", "--eigs-min-good", "--eigs-max-iters", "--eigs-tol", "--eigs-clip", "--eigs-track"};
    const char* lopt[8] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
    static const char* const lname[8] = {"--loop-peak", "--loop-window", "--loop-window-max", "--loop-min-ll-count", "--loop-min-dist", "--loop-max-dist", "--loop-fdr", "--loop-cluster-radius"};
    const char* ilist = nullptr;
    const char* iopt[3] = {nullptr, nullptr, nullptr};
    static const char* const iname[3] = {"--ins-ignore-diags", "--ins-min-frac-valid", "--ins-min-strength"};
    bool apa = false;
    const char* pfile = nullptr;
    const char* popt[4] = {nullptr, nullptr, nullptr, nullptr};              // --pile-edges takes no value: its slot holds the flag itself
    static const char* const pname[4] = {"--pile-flank", "--pile-corner", "--pile-kind", "--pile-edges"};
    bool saddle = false;
    const char* sopt[7] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
    static const char* const sname[7] = {"--saddle-groups", "--saddle-trim", "--saddle-contact", "--saddle-kind", "--saddle-min-dist", "--saddle-max-dist", "--saddle-corner"};
    const char* cfile = nullptr;                                              // --compare
    const char* copt[4] = {nullptr, nullptr, nullptr, nullptr};
    static const char* const cname[4] = {"--scc-h", "--scc-min-dist", "--scc-max-dist", "--scc-weighting"};
    const char* vname = nullptr;                                              // --viewpoint
    bool ebv = false;
    const char* vopt[7] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};     // --vp-second-side takes no value: its slot holds the flag itself
    static const char* const vpname[7] = {"--vp-bin", "--vp-partner-bin", "--vp-track-bin", "--vp-min-count", "--vp-hotspot", "--vp-partners", "--vp-second-side"};
    bool hic = false;                                                         // --hic
    const char* hopt[4] = {nullptr, nullptr, nullptr, nullptr};
    static const char* const hname[4] = {"--hic-level", "--hic-block-bins", "--hic-genome", "--hic-norm-label"};
    const char* bopt[6] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
    static const char* const bname[6] = {"--ignore-diags", "--min-nnz", "--min-count", "--mad-max", "--tol", "--max-iters"};
    for (int i = 1; i < argc; ++i) {
        int b = -1;
        for (int k = 0; k < 6; ++k) if (!strcmp(argv[i], bname[k])) b = k;
        int l = -1;
        for (int k = 0; k < 8; ++k) if (!strcmp(argv[i], lname[k])) l = k;
        int g = -1;
        for (int k = 0; k < 7; ++k) if (!strcmp(argv[i], gname[k])) g = k;
        int s = -1;
        for (int k = 0; k < 3; ++k) if (!strcmp(argv[i], iname[k])) s = k;
        int pl = -1;
        for (int k = 0; k < 4; ++k) if (!strcmp(argv[i], pname[k])) pl = k;
        int sd = -1;
        for (int k = 0; k < 7; ++k) if (!strcmp(argv[i], sname[k])) sd = k;
        int cm = -1;
        for (int k = 0; k < 4; ++k) if (!strcmp(argv[i], cname[k])) cm = k;
        int vp = -1;
        for (int k = 0; k < 7; ++k) if (!strcmp(argv[i], vpname[k])) vp = k;
        int hc = -1;
        for (int k = 0; k < 4; ++k) if (!strcmp(argv[i], hname[k])) hc = k;
        if (hc >= 0) { if (i + 1 >= argc) return usage(argv[0]); hopt[hc] = argv[++i]; }
        else if (!strcmp(argv[i], "--hic")) hic = true;
        else if (vp == 6) vopt[6] = argv[i];
        else if (vp >= 0) { if (i + 1 >= argc) return usage(argv[0]); vopt[vp] = argv[++i]; }
        else if (!strcmp(argv[i], "--viewpoint")) { if (i + 1 >= argc) return usage(argv[0]); vname = argv[++i]; }
        else if (!strcmp(argv[i], "--ebv")) ebv = true;
        else if (cm >= 0) { if (i + 1 >= argc) return usage(argv[0]); copt[cm] = argv[++i]; }
        else if (!strcmp(argv[i], "--compare")) { if (i + 1 >= argc) return usage(argv[0]); cfile = argv[++i]; }
        else if (sd >= 0) { if (i + 1 >= argc) return usage(argv[0]); sopt[sd] = argv[++i]; }
        else if (!strcmp(argv[i], "--saddle")) saddle = eigs = expected = true;
        else if (pl == 3) popt[3] = argv[i];
        else if (pl >= 0) { if (i + 1 >= argc) return usage(argv[0]); popt[pl] = argv[++i]; }
        else if (!strcmp(argv[i], "--apa")) apa = loops = expected = true;
        else if (!strcmp(argv[i], "--pileup")) { if (i + 1 >= argc) return usage(argv[0]); pfile = argv[++i]; expected = true; }
        else if (g >= 0) { if (i + 1 >= argc) return usage(argv[0]); gopt[g] = argv[++i]; }
        else if (s >= 0) { if (i + 1 >= argc) return usage(argv[0]); iopt[s] = argv[++i]; }
        else if (!strcmp(argv[i], "--insulation")) { if (i + 1 >= argc) return usage(argv[0]); ilist = argv[++i]; }
        else if (!strcmp(argv[i], "--eigs")) eigs = expected = true;
        else if (b >= 0) { if (i + 1 >= argc) return usage(argv[0]); bopt[b] = argv[++i]; }
        else if (l >= 0) { if (i + 1 >= argc) return usage(argv[0]); lopt[l] = argv[++i]; }
        else if (!strcmp(argv[i], "--loops")) loops = expected = true;
        else if (!strcmp(argv[i], "--balance")) balance = true;
        else if (!strcmp(argv[i], "--expected")) expected = true;
        else if (!strcmp(argv[i], "-g") && i + 1 < argc) table = argv[++i];
        else if (!strcmp(argv[i], "-r") && i + 1 < argc) rlist = argv[++i];
        else if (!strcmp(argv[i], "-o") && i + 1 < argc) prefix = argv[++i];
        else if (argv[i][0] == '-' && argv[i][1] != '\0') return usage(argv[0]);
        else files.push_back(argv[i]);
    }
    if (!table || !rlist || !prefix) return usage(argv[0]);
    mkt_hic_opts ho;
    mkt_hic_opts_default(&ho);
    for (int k = 0; k < 4; ++k) {
        if (!hopt[k]) continue;
        if (!hic) { fprintf(stderr, "Error: %s needs --hic\n", hname[k]); return usage(argv[0]); }
        if (k >= 2) { (k == 2 ? ho.genome_id : ho.norm_label) = hopt[k]; continue; }
        char* end = nullptr;
        const long v = strtol(hopt[k], &end, 10);
        if (!*hopt[k] || *end || v < 0 || v > 0x7FFFFFFFl) { fprintf(stderr, "Error: %s %s is not a number\n", hname[k], hopt[k]); return 12; }
        if (k == 0) ho.level = (int32_t)v; else ho.block_bins = (uint32_t)v;
    }
    mkt_balance_opts bo;
    mkt_balance_opts_default(&bo);
    for (int k = 0; k < 6; ++k) {
        if (!bopt[k]) continue;
        if (!balance) { fprintf(stderr, "Error: %s needs --balance\n", bname[k]); return usage(argv[0]); }
        const bool ok = k == 0 ? parse_int(bopt[k], bo.ignore_diags) : k == 1 ? parse_int(bopt[k], bo.min_nnz) : k == 2 ? parse_num(bopt[k], bo.min_count)
                      : k == 3 ? parse_num(bopt[k], bo.mad_max) : k == 4 ? parse_num(bopt[k], bo.tol) : (parse_int(bopt[k], bo.max_iters) && bo.max_iters >= 1);
        if (!ok) { fprintf(stderr, "Error: bad value '%s' for %s (%s)\n", bopt[k], bname[k], k == 5 ? "a whole number, at least 1" : k < 2 ? "a whole number, 0 or more" : "a number, 0 or more"); return 12; }
    }
    mkt_loops_opts lo;
    mkt_loops_opts_default(&lo);
    for (int k = 0; k < 8; ++k) {
        if (!lopt[k]) continue;
        if (!loops) { fprintf(stderr, "Error: %s needs --loops\n", lname[k]); return usage(argv[0]); }
        int32_t* const ip[8] = {&lo.peak, &lo.window, &lo.window_max, &lo.min_ll_count, &lo.min_dist, &lo.max_dist, nullptr, &lo.cluster_radius};
        const bool ok = k == 6 ? (parse_num(lopt[k], lo.fdr) && lo.fdr > 0.0 && lo.fdr < 1.0) : parse_int(lopt[k], *ip[k]);
        if (!ok) { fprintf(stderr, "Error: bad value '%s' for %s (%s)\n", lopt[k], lname[k], k == 6 ? "a number inside (0, 1)" : "a whole number, 0 or more"); return 12; }
    }
    // the combinations the library would refuse, before anything is read or written
    if (loops && lo.window <= lo.peak) { fprintf(stderr, "Error: --loop-window %d is not larger than --loop-peak %d\n", lo.window, lo.peak); return 12; }
    if (loops && (lo.window_max < lo.window || lo.window_max > 20)) { fprintf(stderr, "Error: --loop-window-max %d (--loop-window %d .. 20)\n", lo.window_max, lo.window); return 12; }
    mkt_eigs_opts go;
    mkt_eigs_opts_default(&go);
    for (int k = 0; k < 7; ++k) {
        if (!gopt[k]) continue;
        if (!eigs) { fprintf(stderr, "Error: %s needs --eigs\n", gname[k]); return usage(argv[0]); }
        if (k == 6) continue;
        int32_t* const ip[4] = {&go.n_eigs, &go.ignore_diags, &go.min_good, &go.max_iters};
        const bool ok = k == 0 ? (parse_int(gopt[k], go.n_eigs) && go.n_eigs >= 1 && go.n_eigs <= 4) : k < 4 ? parse_int(gopt[k], *ip[k])
                      : k == 4 ? (parse_num(gopt[k], go.tol) && go.tol > 0.0 && go.tol < 1.0) : parse_num(gopt[k], go.clip);
        if (!ok) { fprintf(stderr, "Error: bad value '%s' for %s (%s)\n", gopt[k], gname[k], k == 0 ? "a whole number, 1 .. 4" : k < 4 ? "a whole number, 0 or more" : k == 4 ? "a number inside (0, 1)" : "a number, 0 or more"); return 12; }
    }
    mkt_insulation_opts io;
    mkt_insulation_opts_default(&io);
    io.use_weights = balance ? 1 : 0;
    for (int k = 0; k < 3; ++k) {
        if (!iopt[k]) continue;
        if (!ilist) { fprintf(stderr, "Error: %s needs --insulation\n", iname[k]); return usage(argv[0]); }
        const bool ok = k == 0 ? parse_int(iopt[k], io.ignore_diags) : k == 1 ? (parse_num(iopt[k], io.min_frac_valid) && io.min_frac_valid <= 1.0) : parse_num(iopt[k], io.min_strength);
        if (!ok) { fprintf(stderr, "Error: bad value '%s' for %s (%s)\n", iopt[k], iname[k], k == 0 ? "a whole number, 0 or more" : k == 1 ? "a number inside [0, 1]" : "a number, 0 or more"); return 12; }
    }
    mkt_pileup_opts po;
    mkt_pileup_opts_default(&po);
    for (int k = 0; k < 4; ++k) {
        if (!popt[k]) continue;
        if (!apa && !pfile) { fprintf(stderr, "Error: %s needs --apa or --pileup\n", pname[k]); return usage(argv[0]); }
        bool ok = true;
        if (k == 0) ok = parse_int(popt[k], po.flank) && po.flank >= 1 && po.flank <= 32;
        else if (k == 1) ok = parse_int(popt[k], po.corner) && po.corner >= 1;
        else if (k == 2) {
            if (!strcmp(popt[k], "balanced")) po.kind = MKT_VALUE_BALANCED; else if (!strcmp(popt[k], "oe")) po.kind = MKT_VALUE_OE;
            else if (!strcmp(popt[k], "oe-smooth")) po.kind = MKT_VALUE_OE_SMOOTH; else ok = false;
        } else po.edges = 1;
        if (!ok) { fprintf(stderr, "Error: bad value '%s' for %s (%s)\n", popt[k], pname[k], k == 0 ? "a whole number, 1 .. 32" : k == 1 ? "a whole number, at least 1" : "balanced, oe or oe-smooth"); return 12; }
    }
    if (!popt[1] && po.corner > po.flank) po.corner = po.flank;               // the default corner inside a small window
    if ((apa || pfile) && po.corner > po.flank) { fprintf(stderr, "Error: --pile-corner %d is larger than --pile-flank %d\n", po.corner, po.flank); return 12; }
    mkt_saddle_opts so;
    mkt_saddle_opts_default(&so);
    int32_t sbp[2] = {-1, -1};                                                // --saddle-min-dist, --saddle-max-dist in base pairs
    for (int k = 0; k < 7; ++k) {
        if (!sopt[k]) continue;
        if (!saddle) { fprintf(stderr, "Error: %s needs --saddle\n", sname[k]); return usage(argv[0]); }
        bool ok = true;
        if (k == 0) ok = parse_int(sopt[k], so.n_groups) && so.n_groups >= 2 && so.n_groups <= 64;
        else if (k == 1) {
            const char* comma = strchr(sopt[k], ',');
            ok = comma && parse_int(std::string(sopt[k], comma).c_str(), so.trim_lo) && parse_int(comma + 1, so.trim_hi) && (int64_t)so.trim_lo + so.trim_hi < 10000;
        } else if (k == 2) {
            if (!strcmp(sopt[k], "cis")) so.contact = 0; else if (!strcmp(sopt[k], "trans")) so.contact = 1; else ok = false;
        } else if (k == 3) {
            if (!strcmp(sopt[k], "oe")) so.kind = MKT_VALUE_OE; else if (!strcmp(sopt[k], "oe-smooth")) so.kind = MKT_VALUE_OE_SMOOTH; else ok = false;
        } else if (k < 6) ok = parse_int(sopt[k], sbp[k - 4]);
        else ok = parse_int(sopt[k], so.corner) && so.corner >= 1;
        if (!ok) {
            fprintf(stderr, "Error: bad value '%s' for %s (%s)\n", sopt[k], sname[k], k == 0 ? "a whole number, 2 .. 64" : k == 1 ? "two whole numbers LO,HI, 0 or more, below 10000 together"
                    : k == 2 ? "cis or trans" : k == 3 ? "oe or oe-smooth" : k < 6 ? "a whole number of base pairs, 0 or more" : "a whole number, at least 1");
            return 12;
        }
    }
    if (saddle && so.corner > so.n_groups / 2) { fprintf(stderr, "Error: --saddle-corner %d is larger than half of --saddle-groups %d\n", so.corner, so.n_groups); return 12; }
    if (saddle && sbp[1] > 0 && sbp[1] < sbp[0]) { fprintf(stderr, "Error: --saddle-max-dist %d is below --saddle-min-dist %d\n", sbp[1], sbp[0]); return 12; }
    mkt_scc_opts co;
    mkt_scc_opts_default(&co);
    co.use_weights = balance ? 1 : 0;
    int32_t cbp[2] = {-1, -1};                                                // --scc-min-dist, --scc-max-dist in base pairs
    for (int k = 0; k < 4; ++k) {
        if (!copt[k]) continue;
        if (!cfile) { fprintf(stderr, "Error: %s needs --compare\n", cname[k]); return usage(argv[0]); }
        bool ok = true;
        if (k == 0) ok = parse_int(copt[k], co.h) && co.h <= 16;
        else if (k < 3) ok = parse_int(copt[k], cbp[k - 1]);
        else { if (!strcmp(copt[k], "n")) co.weighting = MKT_SCC_WEIGHT_N; else if (!strcmp(copt[k], "var")) co.weighting = MKT_SCC_WEIGHT_VAR; else ok = false; }
        if (!ok) { fprintf(stderr, "Error: bad value '%s' for %s (%s)\n", copt[k], cname[k], k == 0 ? "a whole number, 0 .. 16" : k < 3 ? "a whole number of base pairs, 0 or more" : "n or var"); return 12; }
    }
    if (cfile && cbp[1] > 0 && cbp[1] < cbp[0]) { fprintf(stderr, "Error: --scc-max-dist %d is below --scc-min-dist %d\n", cbp[1], cbp[0]); return 12; }
    mkt_viewpoint_opts vo;
    mkt_viewpoint_opts_default(&vo);
    int32_t vtrack_bin = 1000;
    std::string vre;                                                          // the partners' expression; empty: every other chromosome
    if (ebv) { if (!vname) vname = "chrEBV"; vre = "chr\\d+$"; vo.second_side_only = 1; vo.min_count = 5; }
    for (int k = 0; k < 7; ++k) {
        if (!vopt[k]) continue;
        if (!vname) { fprintf(stderr, "Error: %s needs --viewpoint or --ebv\n", vpname[k]); return usage(argv[0]); }
        bool ok = true;
        int32_t v = 0;
        if (k < 4) { ok = parse_int(vopt[k], v) && v >= 1; if (ok) { if (k == 0) vo.vbin = (uint32_t)v; else if (k == 1) vo.pbin = (uint32_t)v; else if (k == 2) vtrack_bin = v; else vo.min_count = (uint32_t)v; } }
        else if (k == 4) ok = parse_num(vopt[k], vo.hotspot_ratio) && vo.hotspot_ratio < 1.0;
        else if (k == 5) { vre = vopt[k]; ok = !vre.empty(); }
        else vo.second_side_only = 1;
        if (!ok) { fprintf(stderr, "Error: bad value '%s' for %s (%s)\n", vopt[k], vpname[k], k < 4 ? "a whole number, at least 1" : k == 4 ? "a number inside [0, 1)" : "a regular expression"); return 12; }
    }
    std::vector<uint32_t> ibp;                                                // the windows in base pairs
    if (ilist && (!parse_res(ilist, ibp) || ibp.size() > 4)) { fprintf(stderr, "Error: bad window list '%s' for --insulation (1 .. 4 different positive numbers, comma separated)\n", ilist); return 12; }
    for (size_t k = 1; k < ibp.size(); ++k)
        if (ibp[k] <= ibp[k - 1]) { fprintf(stderr, "Error: the windows of --insulation are not strictly ascending\n"); return 12; }
    std::string ttxt, why;
    if (!read_file(table, ttxt)) { fprintf(stderr, "Error: read chromosome table failed!\n"); return 10; }
    std::vector<Chrom> chroms;
    if (!parse_table(ttxt, chroms, why)) { fprintf(stderr, "Error: bad chromosome table: %s\n", why.c_str()); return 12; }
    std::vector<uint8_t> vmask;                                               // the partners of --viewpoint
    if (vname) {
        size_t v = 0;
        while (v < chroms.size() && chroms[v].name != vname) ++v;
        if (v == chroms.size()) { fprintf(stderr, "Error: --viewpoint %s is not in the chromosome table\n", vname); return 12; }
        vo.viewpoint = (uint32_t)v;
        vmask.assign(chroms.size(), 1);
        if (!vre.empty()) {
            try {
                const std::regex re(vre, std::regex::ECMAScript);
                for (size_t c = 0; c < chroms.size(); ++c) vmask[c] = std::regex_search(chroms[c].name, re) ? 1 : 0;
            } catch (const std::regex_error&) { fprintf(stderr, "Error: bad value '%s' for --vp-partners (a regular expression)\n", vre.c_str()); return 12; }
        }
        vmask[v] = 0;
        size_t np = 0;
        for (uint8_t x : vmask) np += x;
        if (np == 0) { fprintf(stderr, "Error: --vp-partners '%s' keeps no chromosome\n", vre.c_str()); return 12; }
        vo.partner_mask = vmask.data();
    }
    std::vector<uint32_t> res;
    if (!parse_res(rlist, res)) { fprintf(stderr, "Error: bad resolution list '%s' (1 .. 16 different positive numbers, comma separated)\n", rlist); return 12; }
    for (uint32_t r : res)
        for (uint32_t bp : ibp)
            if (bp % r != 0 || bp / r > 1024) { fprintf(stderr, "Error: --insulation window %u is not a multiple of resolution %u of at most 1024 bins\n", bp, r); return 12; }
    for (uint32_t r : res)
        for (int k = 0; k < 2; ++k)
            if (sbp[k] > 0 && (uint32_t)sbp[k] % r != 0) { fprintf(stderr, "Error: %s %d is not a multiple of resolution %u\n", sname[4 + k], sbp[k], r); return 12; }
    for (uint32_t r : res)
        for (int k = 0; k < 2; ++k)
            if (cbp[k] > 0 && (uint32_t)cbp[k] % r != 0) { fprintf(stderr, "Error: %s %d is not a multiple of resolution %u\n", cname[1 + k], cbp[k], r); return 12; }
    if (gopt[6] && res.size() != 1) { fprintf(stderr, "Error: --eigs-track needs a single resolution\n"); return usage(argv[0]); }
    std::vector<double> track;
    if (gopt[6]) {                                                            // the bins of .bins.bed in order, with a value each
        std::string txt;
        if (!read_file(gopt[6], txt)) { fprintf(stderr, "Error: read track file failed!\n"); return 10; }
        size_t p = 0;
        const uint64_t r = res[0];
        for (const Chrom& c : chroms)
            for (uint64_t s0 = 0; s0 < c.len; s0 += r) {
                size_t q = txt.find('\n', p);
                if (p >= txt.size()) { fprintf(stderr, "Error: track file: %zu rows, more bins\n", track.size()); return 12; }
                if (q == std::string::npos) q = txt.size();
                const std::string want = c.name + "\t" + std::to_string(s0) + "\t" + std::to_string(s0 + r < c.len ? s0 + r : c.len) + "\t";
                if (txt.compare(p, want.size(), want) != 0) { fprintf(stderr, "Error: track file row %zu is not bin %s\n", track.size() + 1, want.c_str()); return 12; }
                std::string v = txt.substr(p + want.size(), q - p - want.size());
                if (!v.empty() && v.back() == '\r') v.pop_back();
                char* end = nullptr;
                const double x = strtod(v.c_str(), &end);
                if (v.empty() || *end) { fprintf(stderr, "Error: track file row %zu: '%s' is not a number\n", track.size() + 1, v.c_str()); return 12; }
                track.push_back(x);
                p = q + 1;
            }
        if (p < txt.size()) { fprintf(stderr, "Error: track file has rows past the last bin\n"); return 12; }
    }
    for (uint32_t r : res) {
        uint64_t nb = 0;
        for (const Chrom& c : chroms) nb += (c.len + r - 1) / r;
        if (nb >= (1ull << 32)) { fprintf(stderr, "Error: resolution %u gives 2^32 bins or more\n", r); return 12; }
    }
    std::vector<Anchor> anchors;                                              // the features of --pileup
    if (pfile) {
        std::string txt;
        if (!read_file(pfile, txt)) { fprintf(stderr, "Error: read pileup file failed!\n"); return 10; }
        if (!parse_bedpe(txt, chroms, anchors, why)) { fprintf(stderr, "Error: bad pileup file: %s\n", why.c_str()); return 12; }
    }
    std::vector<FILE*> in;
    for (const char* fn : files) {
        FILE* f = strcmp(fn, "-") ? fopen(fn, "rb") : stdin;
        if (!f) { fprintf(stderr, "Error: read input file failed!\n"); return 10; }
        in.push_back(f);
    }
    if (in.empty()) in.push_back(stdin);
    FILE* cin2 = nullptr;
    if (cfile && !(cin2 = fopen(cfile, "rb"))) { fprintf(stderr, "Error: read input file failed!\n"); return 10; }

    const char* e = getenv("MKT_DEVICE");
    mkt_matrix* m = nullptr;
    int rc = mkt_matrix_create(e ? atoi(e) : 0, ttxt.data(), ttxt.size(), res.data(), (uint32_t)res.size(), &m);
    if (rc == MKT_E_NO_DEVICE) { fprintf(stderr, "Error: GPU matrix: %s\n", mkt_strerror(rc)); return 20; }
    if (rc != MKT_OK) { fprintf(stderr, "Error: GPU matrix: %s: %s\n", mkt_strerror(rc), mkt_matrix_error(nullptr)); return rc == MKT_E_ARG || rc == MKT_E_CAPACITY ? 12 : 21; }
    auto lib_fail = [&](const char* what) { fprintf(stderr, "Error: %s: %s: %s\n", what, mkt_strerror(rc), mkt_matrix_error(m)); mkt_matrix_destroy(m); return 21; };
    std::vector<char> buf((size_t)64 << 20);
    for (FILE* f : in) {
        char last = '\n';
        for (;;) {
            const size_t k = fread(buf.data(), 1, buf.size(), f);
            if (k == 0) break;
            last = buf[k - 1];
            if ((rc = mkt_matrix_add(m, buf.data(), k)) != MKT_OK) return lib_fail("GPU matrix");
        }
        if (ferror(f)) { fprintf(stderr, "Error: read input file failed!\n"); mkt_matrix_destroy(m); return 10; }
        if (f != stdin) fclose(f);
        if (last != '\n' && (rc = mkt_matrix_add(m, "\n", 1)) != MKT_OK) return lib_fail("GPU matrix");      // a file without a final newline does not run into the next one
    }
    uint64_t pairs = 0, skipped = 0;
    if ((rc = mkt_matrix_run(m, &pairs, &skipped)) != MKT_OK) return lib_fail("GPU matrix");
    mkt_matrix* m2 = nullptr;                                                 // the replicate of --compare: the same table and resolutions
    struct Drop { mkt_matrix*& p; ~Drop() { if (p) mkt_matrix_destroy(p); } } drop2{m2};
    auto lib_fail2 = [&](const char* what) { fprintf(stderr, "Error: %s: %s: %s\n", what, mkt_strerror(rc), mkt_matrix_error(m2)); mkt_matrix_destroy(m); return 21; };
    if (cfile) {
        rc = mkt_matrix_create(e ? atoi(e) : 0, ttxt.data(), ttxt.size(), res.data(), (uint32_t)res.size(), &m2);
        if (rc != MKT_OK) { fprintf(stderr, "Error: GPU matrix: %s: %s\n", mkt_strerror(rc), mkt_matrix_error(nullptr)); mkt_matrix_destroy(m); return 21; }
        for (;;) {
            const size_t k = fread(buf.data(), 1, buf.size(), cin2);
            if (k == 0) break;
            if ((rc = mkt_matrix_add(m2, buf.data(), k)) != MKT_OK) return lib_fail2("GPU matrix (--compare)");
        }
        if (ferror(cin2)) { fprintf(stderr, "Error: read input file failed!\n"); mkt_matrix_destroy(m); return 10; }
        fclose(cin2);
        if ((rc = mkt_matrix_run(m2, nullptr, nullptr)) != MKT_OK) return lib_fail2("GPU matrix (--compare)");
    }

    const std::string pre = prefix;
    if (vname) {                                                              // two profiles: the links at --vp-partner-bin, the partner track at --vp-track-bin
        std::vector<std::string> names;
        for (const Chrom& c : chroms) names.push_back(c.name);
        mkt_viewpoint_info vi, ti;
        mkt_viewpoint_opts lo2 = vo;
        lo2.min_count = 1;
        if ((rc = mkt_matrix_viewpoint(m, &lo2, &vi)) != MKT_OK) return lib_fail("GPU viewpoint profile");
        std::vector<mkt::VpLink> links(vi.links);
        std::vector<uint32_t> a(vi.links), b(vi.links), c(vi.links), d(vi.links), track(vi.viewpoint_bins);
        if ((rc = mkt_matrix_fetch_viewpoint_links(m, 0, vi.links, a.data(), b.data(), c.data(), d.data())) != MKT_OK) return lib_fail("GPU viewpoint profile");
        if ((rc = mkt_matrix_fetch_viewpoint_track(m, 0, vi.viewpoint_bins, track.data())) != MKT_OK) return lib_fail("GPU viewpoint profile");
        for (size_t k = 0; k < links.size(); ++k) links[k] = {a[k], b[k], c[k], d[k]};
        const std::string bg = mkt::vp_track_text(track, vname, vo.vbin), lk = mkt::vp_links_text(links, names, vi.min_loop, vo.vbin, vo.pbin);
        mkt_viewpoint_opts to = vo;
        to.pbin = (uint32_t)vtrack_bin;
        if ((rc = mkt_matrix_viewpoint(m, &to, &ti)) != MKT_OK) return lib_fail("GPU viewpoint profile");
        std::vector<mkt::VpCell> cells(ti.partner_cells_kept);
        a.resize(cells.size()); b.resize(cells.size()); c.resize(cells.size());
        if ((rc = mkt_matrix_fetch_viewpoint_partners(m, 0, cells.size(), a.data(), b.data(), c.data())) != MKT_OK) return lib_fail("GPU viewpoint profile");
        for (size_t k = 0; k < cells.size(); ++k) cells[k] = {a[k], b[k], c[k]};
        const std::string pt = mkt::vp_partners_text(cells, names, (uint64_t)vtrack_bin);
        size_t np = 0;
        for (uint8_t x : vmask) np += x;
        std::string vs = std::string("Viewpoint\t") + vname + "\nPartners\t" + std::to_string(np) + "\nSecondSideOnly\t" + std::to_string(vo.second_side_only) + "\nViewpointBin\t" + std::to_string(vo.vbin) +
                         "\nPartnerBin\t" + std::to_string(vo.pbin) + "\nTrackBin\t" + std::to_string(vtrack_bin) + "\nMinCount\t" + std::to_string(vo.min_count) + "\nHotspotRatio\t";
        put_num(vs, vo.hotspot_ratio);
        vs += "\nTotal\t" + std::to_string(vi.total) + "\nLinks\t" + std::to_string(vi.links) + "\nMinLoop\t" + std::to_string(vi.min_loop) + "\nLinksKept\t" + std::to_string(vi.links_kept) +
              "\nViewpointBins\t" + std::to_string(vi.viewpoint_bins) + "\nPartnerCells\t" + std::to_string(ti.partner_cells) + "\nPartnerCellsKept\t" + std::to_string(ti.partner_cells_kept) +
              "\nSkipped\t" + std::to_string(skipped) + "\n";                  // pairs the matrix stage left out: they are absent from the profile
        if (!write_file(pre + ".viewpoint.bedgraph", bg.data(), bg.size()) || !write_file(pre + ".viewpoint.links", lk.data(), lk.size()) || !write_file(pre + ".partners.bedgraph", pt.data(), pt.size()) ||
            !write_file(pre + ".viewpoint.stat", vs.data(), vs.size())) { fprintf(stderr, "Error: write output failed!\n"); mkt_matrix_destroy(m); return 22; }
    }
    std::string bstat, lstat, gstat, istat, astat, pstat, sstat, cstat;
    const uint32_t ni = (uint32_t)ibp.size();
    std::vector<uint64_t> inv;                                                // [ni][nbins] of the resolution at hand
    std::vector<double> isc, ilg, ist;
    std::vector<uint8_t> ibd;
    std::vector<double> evec;
    uint32_t ne = 0;
    std::vector<double> weights;
    std::string stat = "Pairs\t" + std::to_string(pairs) + "\nBinned\t" + std::to_string(pairs - skipped) + "\nSkipped\t" + std::to_string(skipped) + "\n";
    for (uint32_t k = 0; k < res.size(); ++k) {
        uint64_t nbins = 0, nnz = 0, tb = 0;
        if ((rc = mkt_matrix_info(m, k, &nbins, &nnz, &tb)) != MKT_OK) return lib_fail("GPU matrix");
        stat += "nnz." + std::to_string(res[k]) + "\t" + std::to_string(nnz) + "\n";
        const std::string coo = pre + "." + std::to_string(res[k]) + ".coo";
        FILE* f = fopen(coo.c_str(), "wb");
        if (!f) { fprintf(stderr, "Error: write output failed!\n"); mkt_matrix_destroy(m); return 22; }
        for (uint64_t off = 0; off < tb; off += buf.size()) {
            const size_t n = tb - off < buf.size() ? (size_t)(tb - off) : buf.size();
            if ((rc = mkt_matrix_fetch_text(m, k, off, buf.data(), n)) != MKT_OK) { fclose(f); return lib_fail("GPU matrix"); }
            if (fwrite(buf.data(), 1, n, f) != n) { fclose(f); fprintf(stderr, "Error: write output failed!\n"); mkt_matrix_destroy(m); return 22; }
        }
        if (fclose(f) != 0) { fprintf(stderr, "Error: write output failed!\n"); mkt_matrix_destroy(m); return 22; }
        if (balance) {
            mkt_balance_stats bs;
            if ((rc = mkt_matrix_balance(m, k, &bo, &bs)) != MKT_OK) return lib_fail("GPU matrix balance");
            weights.resize(nbins);
            if ((rc = mkt_matrix_fetch_weights(m, k, 0, nbins, weights.data())) != MKT_OK) return lib_fail("GPU matrix balance");
            char line[160];
            snprintf(line, sizeof line, "%u\t%u\t%d\t%.17g\t%.17g\t%llu\n", res[k], bs.iterations, bs.converged, bs.var, bs.scale, (unsigned long long)bs.masked);
            bstat += line;
            if (!bs.converged) fprintf(stderr, "WARN: balancing at resolution %u did not converge in %u iterations (var %g).\n", res[k], bs.iterations, bs.var);
        }
        if (cfile) {
            if (balance && (rc = mkt_matrix_balance(m2, k, &bo, nullptr)) != MKT_OK) return lib_fail2("GPU matrix balance (--compare)");
            co.min_diag = cbp[0] > 0 ? cbp[0] / (int32_t)res[k] : 0;
            if (cbp[1] >= 0) co.max_diag = cbp[1] / (int32_t)res[k];
            else { co.max_diag = (int32_t)(5000000u / res[k]); if (co.max_diag < 1) co.max_diag = 1; if (co.max_diag < co.min_diag) co.max_diag = co.min_diag; }
            mkt_scc_info ci;
            if ((rc = mkt_matrix_scc(m, k, m2, k, &co, &ci)) != MKT_OK) return lib_fail("GPU matrix scc");
            rc = write_scc(m, k, res[k], ci, co.min_diag, chroms, pre + "." + std::to_string(res[k]) + ".scc.tsv", cstat);
            if (rc < 0) { fprintf(stderr, "Error: write output failed!\n"); mkt_matrix_destroy(m); return 22; }
            if (rc != MKT_OK) return lib_fail("GPU matrix scc");
        }
        if (expected) {
            mkt_expected_opts eo;
            mkt_expected_opts_default(&eo);
            eo.use_weights = balance ? 1 : 0;
            mkt_expected_info ei;
            if ((rc = mkt_matrix_expected(m, k, &eo, &ei)) != MKT_OK) return lib_fail("GPU matrix expected");
            const std::string base = pre + "." + std::to_string(res[k]) + ".expected";
            std::vector<uint64_t> nv, cs;
            std::vector<double> bs, ex, sm;
            auto size = [&](uint64_t rows) { nv.resize(rows); cs.resize(rows); bs.resize(rows); ex.resize(rows); sm.resize(rows); };
            auto flush = [&](const std::string& fn, std::string& t, const char*& md, bool last) {      // the first piece truncates, the others append
                if (!last && t.size() <= ((size_t)32 << 20)) return true;
                const bool ok = write_file(fn, t.data(), t.size(), md);
                t.clear(); md = "ab";
                return ok;
            };
            std::string t = "diag\tdist_bp\tn_valid\tcount_sum\tbalanced_sum\texpected\texpected_smooth\n";
            const char* md = "wb";
            bool ok = true;
            size(ei.genome_rows);
            if ((rc = mkt_matrix_fetch_expected_genome(m, k, 0, ei.genome_rows, nv.data(), cs.data(), bs.data(), ex.data(), sm.data())) != MKT_OK) return lib_fail("GPU matrix expected");
            for (uint64_t d = 0; d < ei.genome_rows && ok; ++d) {
                t += std::to_string(d); t += '\t'; t += std::to_string(d * res[k]); t += '\t'; t += std::to_string(nv[d]); t += '\t'; t += std::to_string(cs[d]); t += '\t';
                put_num(t, bs[d]); t += '\t'; put_num(t, ex[d]); t += '\t'; put_num(t, sm[d]); t += '\n';
                ok = flush(base + ".tsv", t, md, false);
            }
            ok = ok && flush(base + ".tsv", t, md, true);
            t = "chrom\tdiag\tn_valid\tcount_sum\tbalanced_sum\n";
            md = "wb";
            size(ei.cis_rows);
            if ((rc = mkt_matrix_fetch_expected_cis(m, k, 0, ei.cis_rows, nv.data(), cs.data(), bs.data())) != MKT_OK) return lib_fail("GPU matrix expected");
            uint64_t row = 0;
            for (const Chrom& c : chroms)
                for (uint64_t d = 0, n = (c.len + res[k] - 1) / res[k]; d < n && ok; ++d, ++row) {
                    t += c.name; t += '\t'; t += std::to_string(d); t += '\t'; t += std::to_string(nv[row]); t += '\t'; t += std::to_string(cs[row]); t += '\t';
                    put_num(t, bs[row]); t += '\n';
                    ok = flush(base + ".chrom.tsv", t, md, false);
                }
            ok = ok && flush(base + ".chrom.tsv", t, md, true);
            t = "chrom1\tchrom2\tn_valid\tcount_sum\tbalanced_sum\texpected\n";
            md = "wb";
            size(ei.trans_rows);
            if ((rc = mkt_matrix_fetch_expected_trans(m, k, 0, ei.trans_rows, nv.data(), cs.data(), bs.data(), ex.data())) != MKT_OK) return lib_fail("GPU matrix expected");
            row = 0;
            for (size_t a = 0; a < chroms.size(); ++a)
                for (size_t b = a + 1; b < chroms.size() && ok; ++b, ++row) {
                    t += chroms[a].name; t += '\t'; t += chroms[b].name; t += '\t'; t += std::to_string(nv[row]); t += '\t'; t += std::to_string(cs[row]); t += '\t';
                    put_num(t, bs[row]); t += '\t'; put_num(t, ex[row]); t += '\n';
                    ok = flush(base + ".trans.tsv", t, md, false);
                }
            ok = ok && flush(base + ".trans.tsv", t, md, true);
            if (!ok) { fprintf(stderr, "Error: write output failed!\n"); mkt_matrix_destroy(m); return 22; }
        }
        if (loops) {
            mkt_loops_info li;
            if ((rc = mkt_matrix_loops(m, k, &lo, &li)) != MKT_OK) return lib_fail("GPU matrix loops");
            std::vector<mkt_loop> rows(li.loops);
            if ((rc = mkt_matrix_fetch_loops(m, k, 0, li.loops, rows.data())) != MKT_OK) return lib_fail("GPU matrix loops");
            lstat += std::to_string(res[k]);
            for (uint64_t v : {li.cells, li.candidates, li.tested, li.undefined, li.over, li.grew, li.at_max, li.enriched, li.loops}) { lstat += '\t'; lstat += std::to_string(v); }
            lstat += '\n';
            std::vector<uint64_t> first;                                          // first bin of every chromosome at this resolution
            uint64_t nb = 0;
            for (const Chrom& c : chroms) { first.push_back(nb); nb += (c.len + res[k] - 1) / res[k]; }
            auto chrom_of = [&](uint64_t bin) { size_t c = chroms.size() - 1; while (first[c] > bin) --c; return c; };
            auto span = [&](std::string& t, size_t c, uint64_t b0, uint64_t b1) {       // start of bin b0 and clipped end of bin b1, both in chromosome c
                const uint64_t s = (b0 - first[c]) * res[k], e = (b1 - first[c] + 1) * res[k];
                t += std::to_string(s); t += '\t'; t += std::to_string(e < chroms[c].len ? e : chroms[c].len);
            };
            std::string t = "#chrom1\tstart1\tend1\tchrom2\tstart2\tend2\tcount\texpected_donut\texpected_ll\texpected_h\texpected_v\twindow\tcells\tbox_start1\tbox_end1\tbox_start2\tbox_end2\n";
            for (const mkt_loop& L : rows) {
                const size_t c = chrom_of(L.bin1);
                t += chroms[c].name; t += '\t'; span(t, c, L.bin1, L.bin1); t += '\t'; t += chroms[c].name; t += '\t'; span(t, c, L.bin2, L.bin2); t += '\t';
                t += std::to_string(L.count);
                for (int R = 0; R < 4; ++R) { t += '\t'; put_num(t, L.r[R]); }
                t += '\t'; t += std::to_string(L.window); t += '\t'; t += std::to_string(L.n_cells); t += '\t';
                span(t, c, L.box[0], L.box[1]); t += '\t'; span(t, c, L.box[2], L.box[3]); t += '\n';
            }
            if (!write_file(pre + "." + std::to_string(res[k]) + ".loops.bedpe", t.data(), t.size())) { fprintf(stderr, "Error: write output failed!\n"); mkt_matrix_destroy(m); return 22; }
            if (apa) {                                                            // the peak cells in loop order
                std::vector<uint32_t> pa, pb;
                for (const mkt_loop& L : rows) { pa.push_back(L.bin1); pb.push_back(L.bin2); }
                mkt_pileup_info pi;
                if ((rc = mkt_matrix_pileup(m, k, pa.data(), pb.data(), pa.size(), &po, &pi)) != MKT_OK) return lib_fail("GPU matrix pileup");
                rc = write_pileup(m, k, res[k], pi, pre + "." + std::to_string(res[k]) + ".apa.tsv", astat);
                if (rc < 0) { fprintf(stderr, "Error: write output failed!\n"); mkt_matrix_destroy(m); return 22; }
                if (rc != MKT_OK) return lib_fail("GPU matrix pileup");
            }
        }
        if (pfile) {
            std::vector<uint64_t> first;
            uint64_t nb = 0;
            for (const Chrom& c : chroms) { first.push_back(nb); nb += (c.len + res[k] - 1) / res[k]; }
            std::vector<uint32_t> pa, pb;
            for (const Anchor& a : anchors) {
                const uint32_t x = (uint32_t)(first[a.c1] + a.m1 / res[k]), y = (uint32_t)(first[a.c2] + a.m2 / res[k]);
                pa.push_back(x < y ? x : y); pb.push_back(x < y ? y : x);
            }
            mkt_pileup_info pi;
            if ((rc = mkt_matrix_pileup(m, k, pa.data(), pb.data(), pa.size(), &po, &pi)) != MKT_OK) return lib_fail("GPU matrix pileup");
            rc = write_pileup(m, k, res[k], pi, pre + "." + std::to_string(res[k]) + ".pileup.tsv", pstat);
            if (rc < 0) { fprintf(stderr, "Error: write output failed!\n"); mkt_matrix_destroy(m); return 22; }
            if (rc != MKT_OK) return lib_fail("GPU matrix pileup");
        }
        if (eigs) {
            mkt_eigs_info gi;
            if ((rc = mkt_matrix_eigs(m, k, &go, track.empty() ? nullptr : track.data(), &gi)) != MKT_OK) return lib_fail("GPU matrix eigs");
            ne = (uint32_t)go.n_eigs;
            evec.resize((size_t)ne * nbins);
            for (uint32_t j = 0; j < ne; ++j)
                if ((rc = mkt_matrix_fetch_eigvecs(m, k, j, 0, nbins, evec.data() + (size_t)j * nbins)) != MKT_OK) return lib_fail("GPU matrix eigs");
            std::vector<double> lam((size_t)gi.n_chrom * ne);
            std::vector<uint32_t> ng(gi.n_chrom), it(gi.n_chrom);
            std::vector<uint8_t> cv(gi.n_chrom);
            if ((rc = mkt_matrix_fetch_eigvals(m, k, 0, gi.n_chrom, lam.data(), nullptr, ng.data(), it.data(), cv.data())) != MKT_OK) return lib_fail("GPU matrix eigs");
            for (uint32_t c = 0; c < gi.n_chrom; ++c) {
                gstat += std::to_string(res[k]); gstat += '\t'; gstat += chroms[c].name; gstat += '\t'; gstat += std::to_string((chroms[c].len + res[k] - 1) / res[k]);
                gstat += '\t'; gstat += std::to_string(ng[c]); gstat += '\t'; gstat += std::to_string(it[c]); gstat += '\t'; gstat += cv[c] ? '1' : '0';
                for (uint32_t j = 0; j < ne; ++j) { gstat += '\t'; put_num(gstat, lam[(size_t)c * ne + j]); }
                gstat += '\n';
                if (it[c] && !cv[c]) fprintf(stderr, "WARN: eigenvectors of %s at resolution %u did not converge in %u iterations.\n", chroms[c].name.c_str(), res[k], it[c]);
            }
            if (saddle) {                                                         // the first vector as the track
                if (sbp[0] >= 0) so.min_diag = sbp[0] / (int32_t)res[k];
                if (sbp[1] >= 0) so.max_diag = sbp[1] / (int32_t)res[k];
                mkt_saddle_info si;
                if ((rc = mkt_matrix_saddle(m, k, &so, evec.data(), &si)) != MKT_OK) return lib_fail("GPU matrix saddle");
                rc = write_saddle(m, k, res[k], si, pre + "." + std::to_string(res[k]) + ".saddle.tsv", sstat);
                if (rc < 0) { fprintf(stderr, "Error: write output failed!\n"); mkt_matrix_destroy(m); return 22; }
                if (rc != MKT_OK) return lib_fail("GPU matrix saddle");
            }
        }
        if (ni) {
            io.n_windows = (int32_t)ni;
            for (uint32_t j = 0; j < 4; ++j) io.window[j] = j < ni ? (int32_t)(ibp[j] / res[k]) : 0;
            mkt_insulation_info ii;
            if ((rc = mkt_matrix_insulation(m, k, &io, &ii)) != MKT_OK) return lib_fail("GPU matrix insulation");
            inv.resize((size_t)ni * nbins); isc.resize((size_t)ni * nbins); ilg.resize((size_t)ni * nbins); ist.resize((size_t)ni * nbins); ibd.resize((size_t)ni * nbins);
            for (uint32_t j = 0; j < ni; ++j) {
                const size_t at = (size_t)j * nbins;
                if ((rc = mkt_matrix_fetch_insulation(m, k, j, 0, nbins, inv.data() + at, nullptr, nullptr, isc.data() + at, ilg.data() + at, ist.data() + at, ibd.data() + at)) != MKT_OK)
                    return lib_fail("GPU matrix insulation");
                istat += std::to_string(res[k]); istat += '\t'; istat += std::to_string(ibp[j]); istat += '\t'; istat += std::to_string(nbins);
                for (uint64_t v : {ii.defined[j], ii.minima[j], ii.boundaries[j]}) { istat += '\t'; istat += std::to_string(v); }
                istat += '\n';
            }
        }
        std::string bed, wbed, gbed, ibed;
        const uint64_t r = res[k];
        const char *mode = "wb", *wmode = "wb", *gmode = "wb", *imode = "wb";     // the first piece truncates, the others append
        if (ni) {
            ibed = "chrom\tstart\tend";
            for (uint32_t j = 0; j < ni; ++j)
                for (const char* col : {"n_valid_", "score_", "log2_insulation_score_", "boundary_strength_", "is_boundary_"}) { ibed += '\t'; ibed += col; ibed += std::to_string(ibp[j]); }
            ibed += '\n';
        }
        if (eigs) { gbed = "chrom\tstart\tend"; for (uint32_t j = 0; j < ne; ++j) { gbed += "\tE"; gbed += std::to_string(j + 1); } gbed += '\n'; }
        uint64_t bin = 0;
        for (const Chrom& c : chroms)
            for (uint64_t s = 0; s < c.len; s += r) {
                const size_t at = bed.size();
                bed += c.name; bed += '\t'; bed += std::to_string(s); bed += '\t'; bed += std::to_string(s + r < c.len ? s + r : c.len); bed += '\n';
                if (balance) {
                    char num[40];
                    const double w = weights[bin];
                    if (w != w) strcpy(num, "nan"); else snprintf(num, sizeof num, "%.17g", w);
                    wbed.append(bed, at, bed.size() - at - 1); wbed += '\t'; wbed += num; wbed += '\n';
                    if (wbed.size() > ((size_t)32 << 20)) {
                        if (!write_file(pre + "." + std::to_string(res[k]) + ".weights.bed", wbed.data(), wbed.size(), wmode)) { fprintf(stderr, "Error: write output failed!\n"); mkt_matrix_destroy(m); return 22; }
                        wbed.clear(); wmode = "ab";
                    }
                }
                if (eigs) {
                    gbed.append(bed, at, bed.size() - at - 1);
                    for (uint32_t j = 0; j < ne; ++j) { gbed += '\t'; put_num(gbed, evec[(size_t)j * nbins + bin]); }
                    gbed += '\n';
                    if (gbed.size() > ((size_t)32 << 20)) {
                        if (!write_file(pre + "." + std::to_string(res[k]) + ".eigs.tsv", gbed.data(), gbed.size(), gmode)) { fprintf(stderr, "Error: write output failed!\n"); mkt_matrix_destroy(m); return 22; }
                        gbed.clear(); gmode = "ab";
                    }
                }
                if (ni) {
                    ibed.append(bed, at, bed.size() - at - 1);
                    for (uint32_t j = 0; j < ni; ++j) {
                        const size_t x = (size_t)j * nbins + bin;
                        ibed += '\t'; ibed += std::to_string(inv[x]); ibed += '\t'; put_num(ibed, isc[x]); ibed += '\t'; put_num(ibed, ilg[x]); ibed += '\t'; put_num(ibed, ist[x]);
                        ibed += ibd[x] ? "\t1" : "\t0";
                    }
                    ibed += '\n';
                    if (ibed.size() > ((size_t)32 << 20)) {
                        if (!write_file(pre + "." + std::to_string(res[k]) + ".insulation.tsv", ibed.data(), ibed.size(), imode)) { fprintf(stderr, "Error: write output failed!\n"); mkt_matrix_destroy(m); return 22; }
                        ibed.clear(); imode = "ab";
                    }
                }
                if (bed.size() > ((size_t)32 << 20)) {
                    if (!write_file(pre + "." + std::to_string(res[k]) + ".bins.bed", bed.data(), bed.size(), mode)) { fprintf(stderr, "Error: write output failed!\n"); mkt_matrix_destroy(m); return 22; }
                    bed.clear(); mode = "ab";
                }
                ++bin;
            }
        if (!write_file(pre + "." + std::to_string(res[k]) + ".bins.bed", bed.data(), bed.size(), mode)) { fprintf(stderr, "Error: write output failed!\n"); mkt_matrix_destroy(m); return 22; }
        if (balance && !write_file(pre + "." + std::to_string(res[k]) + ".weights.bed", wbed.data(), wbed.size(), wmode)) { fprintf(stderr, "Error: write output failed!\n"); mkt_matrix_destroy(m); return 22; }
        if (eigs && !write_file(pre + "." + std::to_string(res[k]) + ".eigs.tsv", gbed.data(), gbed.size(), gmode)) { fprintf(stderr, "Error: write output failed!\n"); mkt_matrix_destroy(m); return 22; }
        if (ni && !write_file(pre + "." + std::to_string(res[k]) + ".insulation.tsv", ibed.data(), ibed.size(), imode)) { fprintf(stderr, "Error: write output failed!\n"); mkt_matrix_destroy(m); return 22; }
    }
    if (hic) {                                                                // every resolution in one container, with the weights of --balance
        mkt_hic_info hi;
        if ((rc = mkt_matrix_hic(m, &ho, &hi)) != MKT_OK) return lib_fail("GPU .hic container");
        std::vector<char> buf((size_t)std::min<uint64_t>(hi.file_bytes, (uint64_t)64 << 20));
        const char* mode = "wb";
        for (uint64_t off = 0; off < hi.file_bytes; off += buf.size()) {
            const size_t n = (size_t)std::min<uint64_t>(buf.size(), hi.file_bytes - off);
            if ((rc = mkt_matrix_fetch_hic(m, off, buf.data(), n)) != MKT_OK) return lib_fail("GPU .hic container");
            if (!write_file(pre + ".hic", buf.data(), n, mode)) { fprintf(stderr, "Error: write output failed!\n"); mkt_matrix_destroy(m); return 22; }
            mode = "ab";
        }
        const std::string hs = "FileBytes\t" + std::to_string(hi.file_bytes) + "\nMatrices\t" + std::to_string(hi.matrices) + "\nBlocks\t" + std::to_string(hi.blocks) +
                               "\nFloatBlocks\t" + std::to_string(hi.float_blocks) + "\nPieces\t" + std::to_string(hi.pieces) + "\nRawBytes\t" + std::to_string(hi.raw_bytes) +
                               "\nDeflatedBytes\t" + std::to_string(hi.deflated_bytes) + "\nLevel\t" + std::to_string(ho.level) + "\nBlockBins\t" + std::to_string(ho.block_bins) + "\n";
        if (!write_file(pre + ".hic.stat", hs.data(), hs.size())) { fprintf(stderr, "Error: write output failed!\n"); mkt_matrix_destroy(m); return 22; }
    }
    if (cfile && !write_file(pre + ".scc.stat", cstat.data(), cstat.size())) { fprintf(stderr, "Error: write output failed!\n"); mkt_matrix_destroy(m); return 22; }
    if (saddle && !write_file(pre + ".saddle.stat", sstat.data(), sstat.size())) { fprintf(stderr, "Error: write output failed!\n"); mkt_matrix_destroy(m); return 22; }
    if (apa && !write_file(pre + ".apa.stat", astat.data(), astat.size())) { fprintf(stderr, "Error: write output failed!\n"); mkt_matrix_destroy(m); return 22; }
    if (pfile && !write_file(pre + ".pileup.stat", pstat.data(), pstat.size())) { fprintf(stderr, "Error: write output failed!\n"); mkt_matrix_destroy(m); return 22; }
    if (ni && !write_file(pre + ".insulation.stat", istat.data(), istat.size())) { fprintf(stderr, "Error: write output failed!\n"); mkt_matrix_destroy(m); return 22; }
    if (eigs && !write_file(pre + ".eigs.stat", gstat.data(), gstat.size())) { fprintf(stderr, "Error: write output failed!\n"); mkt_matrix_destroy(m); return 22; }
    if (balance && !write_file(pre + ".balance.stat", bstat.data(), bstat.size())) { fprintf(stderr, "Error: write output failed!\n"); mkt_matrix_destroy(m); return 22; }
    if (loops && !write_file(pre + ".loops.stat", lstat.data(), lstat.size())) { fprintf(stderr, "Error: write output failed!\n"); mkt_matrix_destroy(m); return 22; }
    if (!write_file(pre + ".matrix.stat", stat.data(), stat.size())) { fprintf(stderr, "Error: write output failed!\n"); mkt_matrix_destroy(m); return 22; }
    mkt_matrix_destroy(m);
    return 0;
}
