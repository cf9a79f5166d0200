// pairs2matrix -- the computation behind the driver's last stage (microcket:520-554: `juicer_tools pre -r 2500000,...,5000` and
// `cooler cload pairix GINFO:minBIN`) on the GPU: final.pairs -> the sparse binned contact matrix at every resolution asked for.
// The .hic / .cool containers themselves are not written; the output is what `cooler load -f coo <chrom.sizes>:<r>` ingests.
// The work is mkt_matrix_* of libmkt_hip.so (include/mkt.h, where the binning is defined); this file only moves bytes.
//
//   pairs2matrix -g <chrom.sizes> -r r1[,r2,...] -o <prefix> [in.pairs ...]        (no input file: stdin; $MKT_DEVICE: GPU ordinal)
//                an input (and --compare OTHER) that begins with the gzip magic bytes is read as BGZF and inflated on the device
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
#include <algorithm>
#include <cerrno>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <functional>
#include <initializer_list>
#include <memory>
#include <regex>
#include <string>
#include <utility>
#include <vector>
#include "../../include/mkt.h"
#include "mkt_chunked_file.h"
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
using mkt::ChunkedFile;
using mkt::write_file;

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

// ---- the command line ---------------------------------------------------------------------------------------------------------------
// One row per option: its name, its group and whether it takes a value.  scan() is one loop over the table; everything after it names an
// option by its id.  A group is on when one of its switches is given; a sub-option of a group that is off is a usage error.
enum Opt {
    O_TABLE, O_RES, O_PREFIX, O_BALANCE, O_EXPECTED, O_LOOPS, O_EIGS, O_INSULATION, O_APA, O_PILEUP, O_SADDLE, O_COMPARE, O_VIEWPOINT, O_EBV, O_HIC,
    O_HIC_LEVEL, O_HIC_BLOCK_BINS, O_HIC_GENOME, O_HIC_NORM_LABEL,
    O_IGNORE_DIAGS, O_MIN_NNZ, O_MIN_COUNT, O_MAD_MAX, O_TOL, O_MAX_ITERS,
    O_LOOP_PEAK, O_LOOP_WINDOW, O_LOOP_WINDOW_MAX, O_LOOP_MIN_LL_COUNT, O_LOOP_MIN_DIST, O_LOOP_MAX_DIST, O_LOOP_FDR, O_LOOP_CLUSTER_RADIUS,
    O_EIGS_N, O_EIGS_IGNORE_DIAGS, O_EIGS_MIN_GOOD, O_EIGS_MAX_ITERS, O_EIGS_TOL, O_EIGS_CLIP, O_EIGS_TRACK,
    O_INS_IGNORE_DIAGS, O_INS_MIN_FRAC_VALID, O_INS_MIN_STRENGTH,
    O_PILE_FLANK, O_PILE_CORNER, O_PILE_KIND, O_PILE_EDGES,
    O_SADDLE_GROUPS, O_SADDLE_TRIM, O_SADDLE_CONTACT, O_SADDLE_KIND, O_SADDLE_MIN_DIST, O_SADDLE_MAX_DIST, O_SADDLE_CORNER,
    O_SCC_H, O_SCC_MIN_DIST, O_SCC_MAX_DIST, O_SCC_WEIGHTING,
    O_VP_BIN, O_VP_PARTNER_BIN, O_VP_TRACK_BIN, O_VP_MIN_COUNT, O_VP_HOTSPOT, O_VP_PARTNERS, O_VP_SECOND_SIDE,
    N_OPTS
};
enum Group { G_MAIN, G_HIC, G_BALANCE, G_LOOPS, G_EIGS, G_INSULATION, G_PILEUP, G_SADDLE, G_SCC, G_VIEWPOINT };
struct OptRow { Opt id; const char* name; Group group; bool takes_value; };
static constexpr OptRow OPTS[N_OPTS] = {
    {O_TABLE, "-g", G_MAIN, true}, {O_RES, "-r", G_MAIN, true}, {O_PREFIX, "-o", G_MAIN, true},
    {O_BALANCE, "--balance", G_MAIN, false}, {O_EXPECTED, "--expected", G_MAIN, false}, {O_LOOPS, "--loops", G_MAIN, false}, {O_EIGS, "--eigs", G_MAIN, false},
    {O_INSULATION, "--insulation", G_MAIN, true}, {O_APA, "--apa", G_MAIN, false}, {O_PILEUP, "--pileup", G_MAIN, true}, {O_SADDLE, "--saddle", G_MAIN, false},
    {O_COMPARE, "--compare", G_MAIN, true}, {O_VIEWPOINT, "--viewpoint", G_MAIN, true}, {O_EBV, "--ebv", G_MAIN, false}, {O_HIC, "--hic", G_MAIN, false},
    {O_HIC_LEVEL, "--hic-level", G_HIC, true}, {O_HIC_BLOCK_BINS, "--hic-block-bins", G_HIC, true}, {O_HIC_GENOME, "--hic-genome", G_HIC, true},
    {O_HIC_NORM_LABEL, "--hic-norm-label", G_HIC, true},
    {O_IGNORE_DIAGS, "--ignore-diags", G_BALANCE, true}, {O_MIN_NNZ, "--min-nnz", G_BALANCE, true}, {O_MIN_COUNT, "--min-count", G_BALANCE, true},
    {O_MAD_MAX, "--mad-max", G_BALANCE, true}, {O_TOL, "--tol", G_BALANCE, true}, {O_MAX_ITERS, "--max-iters", G_BALANCE, true},
    {O_LOOP_PEAK, "--loop-peak", G_LOOPS, true}, {O_LOOP_WINDOW, "--loop-window", G_LOOPS, true}, {O_LOOP_WINDOW_MAX, "--loop-window-max", G_LOOPS, true},
    {O_LOOP_MIN_LL_COUNT, "--loop-min-ll-count", G_LOOPS, true}, {O_LOOP_MIN_DIST, "--loop-min-dist", G_LOOPS, true}, {O_LOOP_MAX_DIST, "--loop-max-dist", G_LOOPS, true},
    {O_LOOP_FDR, "--loop-fdr", G_LOOPS, true}, {O_LOOP_CLUSTER_RADIUS, "--loop-cluster-radius", G_LOOPS, true},
    {O_EIGS_N, "--eigs-n", G_EIGS, true}, {O_EIGS_IGNORE_DIAGS, "--eigs-ignore-diags", G_EIGS, true}, {O_EIGS_MIN_GOOD, "--eigs-min-good", G_EIGS, true},
    {O_EIGS_MAX_ITERS, "--eigs-max-iters", G_EIGS, true}, {O_EIGS_TOL, "--eigs-tol", G_EIGS, true}, {O_EIGS_CLIP, "--eigs-clip", G_EIGS, true},
    {O_EIGS_TRACK, "--eigs-track", G_EIGS, true},
    {O_INS_IGNORE_DIAGS, "--ins-ignore-diags", G_INSULATION, true}, {O_INS_MIN_FRAC_VALID, "--ins-min-frac-valid", G_INSULATION, true},
    {O_INS_MIN_STRENGTH, "--ins-min-strength", G_INSULATION, true},
    {O_PILE_FLANK, "--pile-flank", G_PILEUP, true}, {O_PILE_CORNER, "--pile-corner", G_PILEUP, true}, {O_PILE_KIND, "--pile-kind", G_PILEUP, true},
    {O_PILE_EDGES, "--pile-edges", G_PILEUP, false},
    {O_SADDLE_GROUPS, "--saddle-groups", G_SADDLE, true}, {O_SADDLE_TRIM, "--saddle-trim", G_SADDLE, true}, {O_SADDLE_CONTACT, "--saddle-contact", G_SADDLE, true},
    {O_SADDLE_KIND, "--saddle-kind", G_SADDLE, true}, {O_SADDLE_MIN_DIST, "--saddle-min-dist", G_SADDLE, true}, {O_SADDLE_MAX_DIST, "--saddle-max-dist", G_SADDLE, true},
    {O_SADDLE_CORNER, "--saddle-corner", G_SADDLE, true},
    {O_SCC_H, "--scc-h", G_SCC, true}, {O_SCC_MIN_DIST, "--scc-min-dist", G_SCC, true}, {O_SCC_MAX_DIST, "--scc-max-dist", G_SCC, true},
    {O_SCC_WEIGHTING, "--scc-weighting", G_SCC, true},
    {O_VP_BIN, "--vp-bin", G_VIEWPOINT, true}, {O_VP_PARTNER_BIN, "--vp-partner-bin", G_VIEWPOINT, true}, {O_VP_TRACK_BIN, "--vp-track-bin", G_VIEWPOINT, true},
    {O_VP_MIN_COUNT, "--vp-min-count", G_VIEWPOINT, true}, {O_VP_HOTSPOT, "--vp-hotspot", G_VIEWPOINT, true}, {O_VP_PARTNERS, "--vp-partners", G_VIEWPOINT, true},
    {O_VP_SECOND_SIDE, "--vp-second-side", G_VIEWPOINT, false},
};
constexpr bool opts_in_order() { for (int o = 0; o < N_OPTS; ++o) if (OPTS[o].id != o) return false; return true; }
static_assert(opts_in_order(), "OPTS lists the options in the order of enum Opt");
// the switches of a group, by Group: the second is N_OPTS where there is one only
static constexpr Opt SWITCHES[][2] = {{N_OPTS, N_OPTS}, {O_HIC, N_OPTS}, {O_BALANCE, N_OPTS}, {O_LOOPS, N_OPTS}, {O_EIGS, N_OPTS}, {O_INSULATION, N_OPTS}, {O_APA, O_PILEUP},
                                      {O_SADDLE, N_OPTS}, {O_COMPARE, N_OPTS}, {O_VIEWPOINT, O_EBV}};
// a switch that turns another on
static constexpr Opt IMPLIES[][2] = {{O_SADDLE, O_EIGS}, {O_SADDLE, O_EXPECTED}, {O_APA, O_LOOPS}, {O_APA, O_EXPECTED}, {O_PILEUP, O_EXPECTED}, {O_EIGS, O_EXPECTED},
                                     {O_LOOPS, O_EXPECTED}};

struct Args {
    const char* me = nullptr;
    const char* val[N_OPTS] = {};                    // the value of an option, the option itself for one that takes none; nullptr: not given, not implied
    std::vector<const char*> files;
    bool on(Opt o) const { return val[o] != nullptr; }
};
static const char* name(Opt o) { return OPTS[o].name; }

// argv -> a; the last of a repeated option holds.  Anything else that begins with '-' and is not "-" alone is a usage error.
static int scan(int argc, char* argv[], Args& a) {
    a.me = argv[0];
    for (int i = 1; i < argc; ++i) {
        int o = 0;
        while (o < N_OPTS && strcmp(argv[i], OPTS[o].name)) ++o;
        if (o < N_OPTS && !OPTS[o].takes_value) a.val[o] = argv[i];
        else if (o < N_OPTS) { if (i + 1 >= argc) return usage(a.me); a.val[o] = argv[++i]; }
        else if (argv[i][0] == '-' && argv[i][1] != '\0') return usage(a.me);
        else a.files.push_back(argv[i]);
    }
    if (!a.on(O_TABLE) || !a.on(O_RES) || !a.on(O_PREFIX)) return usage(a.me);
    for (const auto& p : IMPLIES) if (a.on(p[0]) && !a.on(p[1])) a.val[p[1]] = name(p[1]);
    return 0;
}

// 0 when the group of sub-option o is on, otherwise the usage error
static int needs_switch(const Args& a, Opt o) {
    const Opt s = SWITCHES[OPTS[o].group][0], s2 = SWITCHES[OPTS[o].group][1];
    if (a.on(s) || (s2 != N_OPTS && a.on(s2))) return 0;
    if (s2 == N_OPTS) fprintf(stderr, "Error: %s needs %s\n", name(o), name(s)); else fprintf(stderr, "Error: %s needs %s or %s\n", name(o), name(s), name(s2));
    return usage(a.me);
}
// A sub-option with where its value goes and what a good one is.  apply() takes the given ones of a group in the order of the rows, which
// is the order their errors are reported in: 2 for one whose group is off, 12 for a value that set() refuses.
struct Row { Opt o; std::function<bool(const char*)> set; const char* what; };
static int apply(const Args& a, std::initializer_list<Row> rows) {
    for (const Row& r : rows) {
        if (!a.on(r.o)) continue;
        if (const int rc = needs_switch(a, r.o)) return rc;
        if (!r.set(a.val[r.o])) { fprintf(stderr, "Error: bad value '%s' for %s (%s)\n", a.val[r.o], name(r.o), r.what); return 12; }
    }
    return 0;
}
static const char WHOLE[] = "a whole number, 0 or more", AT_LEAST_1[] = "a whole number, at least 1", BASE_PAIRS[] = "a whole number of base pairs, 0 or more";
static const char NUMBER[] = "a number, 0 or more", INSIDE_0_1[] = "a number inside (0, 1)";
static Row whole(Opt o, int32_t& to, const char* what = WHOLE, int32_t lo = 0, int32_t hi = 0x7FFFFFFF) {
    return {o, [&to, lo, hi](const char* s) { return parse_int(s, to) && to >= lo && to <= hi; }, what};
}
static Row whole_u32(Opt o, uint32_t& to, const char* what, int32_t lo) {                 // `to` is left alone by a value that is refused
    return {o, [&to, lo](const char* s) { int32_t v = 0; if (!parse_int(s, v) || v < lo) return false; to = (uint32_t)v; return true; }, what};
}
static Row number(Opt o, double& to, const char* what = NUMBER, bool (*good)(double) = nullptr) {
    return {o, [&to, good](const char* s) { return parse_num(s, to) && (!good || good(to)); }, what};
}
static Row one_of(Opt o, int32_t& to, std::initializer_list<std::pair<const char*, int32_t>> words, const char* what) {
    const std::vector<std::pair<const char*, int32_t>> w(words);
    return {o, [&to, w](const char* s) { for (const auto& x : w) if (!strcmp(s, x.first)) { to = x.second; return true; } return false; }, what};
}
static bool inside_0_1(double v) { return v > 0.0 && v < 1.0; }

// ---- the run: what the command line said, the two matrices, and the one way out of a failure -----------------------------------------
struct CloseFile { void operator()(FILE* f) const { if (f != stdin) fclose(f); } };
typedef std::unique_ptr<FILE, CloseFile> File;
struct Matrix {                                      // owns a mkt_matrix
    mkt_matrix* p = nullptr;
    Matrix() {}
    Matrix(const Matrix&) = delete;
    Matrix& operator=(const Matrix&) = delete;
    ~Matrix() { if (p) mkt_matrix_destroy(p); }
    operator mkt_matrix*() const { return p; }
};
struct Run {
    Args a;
    mkt_hic_opts ho; mkt_balance_opts bo; mkt_loops_opts lo; mkt_eigs_opts go; mkt_insulation_opts io; mkt_pileup_opts po; mkt_saddle_opts so; mkt_scc_opts co; mkt_viewpoint_opts vo;
    int32_t sbp[2] = {-1, -1}, cbp[2] = {-1, -1};    // min-dist, max-dist of saddle and of scc in base pairs: divided per resolution
    const char* vname = nullptr;                     // the viewpoint
    int32_t vtrack_bin = 1000;
    std::string vre;                                 // the partners' expression; empty: every other chromosome
    std::vector<uint8_t> vmask;                      // the partners
    std::vector<uint32_t> ibp;                       // the windows of insulation in base pairs
    std::vector<double> track;                       // the orienting track of the eigenvectors
    std::vector<Anchor> anchors;                     // the features of the pileup file
    std::string ttxt, pre;
    std::vector<Chrom> chroms;
    std::vector<uint32_t> res;
    std::vector<File> in;
    File in2;
    Matrix m2, m;                                    // m2: the replicate to compare with; destroyed after m
    int rc = MKT_OK;                                 // of the last library call
    uint64_t pairs = 0, skipped = 0;
    std::vector<char> buf;
    // per bin of the resolution at hand, from its analyses to the per-bin files
    std::vector<double> weights, evec, isc, ilg, ist;
    std::vector<uint64_t> inv;
    std::vector<uint8_t> ibd;
    uint32_t ne = 0;
    std::string stat, bstat, lstat, gstat, istat, astat, pstat, sstat, cstat;

    bool ok(int r) { rc = r; return r == MKT_OK; }
    int fail_lib(const char* what, bool compare = false) const {
        fprintf(stderr, "Error: %s%s: %s: %s\n", what, compare ? " (--compare)" : "", mkt_strerror(rc), mkt_matrix_error(compare ? m2 : m));
        return 21;
    }
    int fail_write() const { fprintf(stderr, "Error: write output failed!\n"); return 22; }
    int fail_read() const { fprintf(stderr, "Error: read input file failed!\n"); return 10; }
};
// one resolution of the run
struct Level {
    uint32_t k, r;
    uint64_t nbins;
    std::string base;                                // <prefix>.<r>
    std::vector<uint64_t> first;                     // first bin of every chromosome
};
static size_t chrom_of(const Level& L, uint64_t bin) { size_t c = L.first.size() - 1; while (L.first[c] > bin) --c; return c; }
// start of bin b0 and clipped end of bin b1, both in chromosome c
static void span(std::string& t, const Run& R, const Level& L, size_t c, uint64_t b0, uint64_t b1) {
    const uint64_t s = (b0 - L.first[c]) * L.r, e = (b1 - L.first[c] + 1) * L.r;
    t += std::to_string(s); t += '\t'; t += std::to_string(e < R.chroms[c].len ? e : R.chroms[c].len);
}

// ---- the options of each group: 0, 2 (usage) or 12 (bad value) -------------------------------------------------------------------------
static int hic_options(Run& R) {
    mkt_hic_opts_default(&R.ho);
    for (Opt o : {O_HIC_LEVEL, O_HIC_BLOCK_BINS, O_HIC_GENOME, O_HIC_NORM_LABEL}) {
        const char* v = R.a.val[o];
        if (!v) continue;
        if (const int rc = needs_switch(R.a, o)) return rc;
        if (o == O_HIC_GENOME) { R.ho.genome_id = v; continue; }
        if (o == O_HIC_NORM_LABEL) { R.ho.norm_label = v; continue; }
        char* end = nullptr;
        const long x = strtol(v, &end, 10);
        if (!*v || *end || x < 0 || x > 0x7FFFFFFFl) { fprintf(stderr, "Error: %s %s is not a number\n", name(o), v); return 12; }
        if (o == O_HIC_LEVEL) R.ho.level = (int32_t)x; else R.ho.block_bins = (uint32_t)x;
    }
    return 0;
}
static int balance_options(Run& R) {
    mkt_balance_opts& bo = R.bo;
    mkt_balance_opts_default(&bo);
    return apply(R.a, {whole(O_IGNORE_DIAGS, bo.ignore_diags), whole(O_MIN_NNZ, bo.min_nnz), number(O_MIN_COUNT, bo.min_count), number(O_MAD_MAX, bo.mad_max), number(O_TOL, bo.tol),
                       whole(O_MAX_ITERS, bo.max_iters, AT_LEAST_1, 1)});
}
static int loops_options(Run& R) {
    mkt_loops_opts& lo = R.lo;
    mkt_loops_opts_default(&lo);
    if (const int rc = apply(R.a, {whole(O_LOOP_PEAK, lo.peak), whole(O_LOOP_WINDOW, lo.window), whole(O_LOOP_WINDOW_MAX, lo.window_max), whole(O_LOOP_MIN_LL_COUNT, lo.min_ll_count),
                                   whole(O_LOOP_MIN_DIST, lo.min_dist), whole(O_LOOP_MAX_DIST, lo.max_dist), number(O_LOOP_FDR, lo.fdr, INSIDE_0_1, inside_0_1),
                                   whole(O_LOOP_CLUSTER_RADIUS, lo.cluster_radius)})) return rc;
    // the combinations the library would refuse, before anything is read or written
    if (R.a.on(O_LOOPS) && lo.window <= lo.peak) { fprintf(stderr, "Error: %s %d is not larger than %s %d\n", name(O_LOOP_WINDOW), lo.window, name(O_LOOP_PEAK), lo.peak); return 12; }
    if (R.a.on(O_LOOPS) && (lo.window_max < lo.window || lo.window_max > 20)) {
        fprintf(stderr, "Error: %s %d (%s %d .. 20)\n", name(O_LOOP_WINDOW_MAX), lo.window_max, name(O_LOOP_WINDOW), lo.window);
        return 12;
    }
    return 0;
}
static int eigs_options(Run& R) {
    mkt_eigs_opts& go = R.go;
    mkt_eigs_opts_default(&go);
    return apply(R.a, {whole(O_EIGS_N, go.n_eigs, "a whole number, 1 .. 4", 1, 4), whole(O_EIGS_IGNORE_DIAGS, go.ignore_diags), whole(O_EIGS_MIN_GOOD, go.min_good),
                       whole(O_EIGS_MAX_ITERS, go.max_iters), number(O_EIGS_TOL, go.tol, INSIDE_0_1, inside_0_1), number(O_EIGS_CLIP, go.clip),
                       {O_EIGS_TRACK, [](const char*) { return true; }, ""}});             // read once the bins are known: read_track()
}
static int insulation_options(Run& R) {
    mkt_insulation_opts& io = R.io;
    mkt_insulation_opts_default(&io);
    io.use_weights = R.a.on(O_BALANCE) ? 1 : 0;
    return apply(R.a, {whole(O_INS_IGNORE_DIAGS, io.ignore_diags), number(O_INS_MIN_FRAC_VALID, io.min_frac_valid, "a number inside [0, 1]", [](double v) { return v <= 1.0; }),
                       number(O_INS_MIN_STRENGTH, io.min_strength)});
}
static int pileup_options(Run& R) {
    mkt_pileup_opts& po = R.po;
    mkt_pileup_opts_default(&po);
    if (const int rc = apply(R.a, {whole(O_PILE_FLANK, po.flank, "a whole number, 1 .. 32", 1, 32), whole(O_PILE_CORNER, po.corner, AT_LEAST_1, 1),
                                   one_of(O_PILE_KIND, po.kind, {{"balanced", MKT_VALUE_BALANCED}, {"oe", MKT_VALUE_OE}, {"oe-smooth", MKT_VALUE_OE_SMOOTH}}, "balanced, oe or oe-smooth"),
                                   {O_PILE_EDGES, [&po](const char*) { po.edges = 1; return true; }, ""}})) return rc;
    if (!R.a.on(O_PILE_CORNER) && po.corner > po.flank) po.corner = po.flank;             // the default corner inside a small window
    if ((R.a.on(O_APA) || R.a.on(O_PILEUP)) && po.corner > po.flank) {
        fprintf(stderr, "Error: %s %d is larger than %s %d\n", name(O_PILE_CORNER), po.corner, name(O_PILE_FLANK), po.flank);
        return 12;
    }
    return 0;
}
static int saddle_options(Run& R) {
    mkt_saddle_opts& so = R.so;
    mkt_saddle_opts_default(&so);
    const auto trim = [&so](const char* s) {
        const char* comma = strchr(s, ',');
        return comma && parse_int(std::string(s, comma).c_str(), so.trim_lo) && parse_int(comma + 1, so.trim_hi) && (int64_t)so.trim_lo + so.trim_hi < 10000;
    };
    if (const int rc = apply(R.a, {whole(O_SADDLE_GROUPS, so.n_groups, "a whole number, 2 .. 64", 2, 64), {O_SADDLE_TRIM, trim, "two whole numbers LO,HI, 0 or more, below 10000 together"},
                                   one_of(O_SADDLE_CONTACT, so.contact, {{"cis", 0}, {"trans", 1}}, "cis or trans"),
                                   one_of(O_SADDLE_KIND, so.kind, {{"oe", MKT_VALUE_OE}, {"oe-smooth", MKT_VALUE_OE_SMOOTH}}, "oe or oe-smooth"),
                                   whole(O_SADDLE_MIN_DIST, R.sbp[0], BASE_PAIRS), whole(O_SADDLE_MAX_DIST, R.sbp[1], BASE_PAIRS), whole(O_SADDLE_CORNER, so.corner, AT_LEAST_1, 1)})) return rc;
    if (R.a.on(O_SADDLE) && so.corner > so.n_groups / 2) {
        fprintf(stderr, "Error: %s %d is larger than half of %s %d\n", name(O_SADDLE_CORNER), so.corner, name(O_SADDLE_GROUPS), so.n_groups);
        return 12;
    }
    if (R.a.on(O_SADDLE) && R.sbp[1] > 0 && R.sbp[1] < R.sbp[0]) { fprintf(stderr, "Error: %s %d is below %s %d\n", name(O_SADDLE_MAX_DIST), R.sbp[1], name(O_SADDLE_MIN_DIST), R.sbp[0]); return 12; }
    return 0;
}
static int scc_options(Run& R) {
    mkt_scc_opts& co = R.co;
    mkt_scc_opts_default(&co);
    co.use_weights = R.a.on(O_BALANCE) ? 1 : 0;
    if (const int rc = apply(R.a, {whole(O_SCC_H, co.h, "a whole number, 0 .. 16", 0, 16), whole(O_SCC_MIN_DIST, R.cbp[0], BASE_PAIRS), whole(O_SCC_MAX_DIST, R.cbp[1], BASE_PAIRS),
                                   one_of(O_SCC_WEIGHTING, co.weighting, {{"n", MKT_SCC_WEIGHT_N}, {"var", MKT_SCC_WEIGHT_VAR}}, "n or var")})) return rc;
    if (R.a.on(O_COMPARE) && R.cbp[1] > 0 && R.cbp[1] < R.cbp[0]) { fprintf(stderr, "Error: %s %d is below %s %d\n", name(O_SCC_MAX_DIST), R.cbp[1], name(O_SCC_MIN_DIST), R.cbp[0]); return 12; }
    return 0;
}
static int viewpoint_options(Run& R) {
    mkt_viewpoint_opts& vo = R.vo;
    mkt_viewpoint_opts_default(&vo);
    R.vname = R.a.val[O_VIEWPOINT];
    if (R.a.on(O_EBV)) { if (!R.vname) R.vname = "chrEBV"; R.vre = "chr\\d+$"; vo.second_side_only = 1; vo.min_count = 5; }      // the preset first: each option still overrides
    return apply(R.a, {whole_u32(O_VP_BIN, vo.vbin, AT_LEAST_1, 1), whole_u32(O_VP_PARTNER_BIN, vo.pbin, AT_LEAST_1, 1), whole(O_VP_TRACK_BIN, R.vtrack_bin, AT_LEAST_1, 1),
                       whole_u32(O_VP_MIN_COUNT, vo.min_count, AT_LEAST_1, 1), number(O_VP_HOTSPOT, vo.hotspot_ratio, "a number inside [0, 1)", [](double v) { return v < 1.0; }),
                       {O_VP_PARTNERS, [&R](const char* s) { R.vre = s; return !R.vre.empty(); }, "a regular expression"},
                       {O_VP_SECOND_SIDE, [&vo](const char*) { vo.second_side_only = 1; return true; }, ""}});
}

// ---- what is checked after the options, in this order, before a device is asked for --------------------------------------------------
static int insulation_windows(Run& R) {
    const char* list = R.a.val[O_INSULATION];
    if (list && (!parse_res(list, R.ibp) || R.ibp.size() > 4)) {
        fprintf(stderr, "Error: bad window list '%s' for %s (1 .. 4 different positive numbers, comma separated)\n", list, name(O_INSULATION));
        return 12;
    }
    for (size_t k = 1; k < R.ibp.size(); ++k)
        if (R.ibp[k] <= R.ibp[k - 1]) { fprintf(stderr, "Error: the windows of %s are not strictly ascending\n", name(O_INSULATION)); return 12; }
    return 0;
}
static int read_table(Run& R) {
    std::string why;
    if (!read_file(R.a.val[O_TABLE], R.ttxt)) { fprintf(stderr, "Error: read chromosome table failed!\n"); return 10; }
    if (!parse_table(R.ttxt, R.chroms, why)) { fprintf(stderr, "Error: bad chromosome table: %s\n", why.c_str()); return 12; }
    return 0;
}
// the viewpoint's index and the mask of its partners
static int viewpoint_partners(Run& R) {
    if (!R.vname) return 0;
    const std::vector<Chrom>& chroms = R.chroms;
    size_t v = 0;
    while (v < chroms.size() && chroms[v].name != R.vname) ++v;
    if (v == chroms.size()) { fprintf(stderr, "Error: %s %s is not in the chromosome table\n", name(O_VIEWPOINT), R.vname); return 12; }
    R.vo.viewpoint = (uint32_t)v;
    R.vmask.assign(chroms.size(), 1);
    if (!R.vre.empty()) {
        try {
            const std::regex re(R.vre, std::regex::ECMAScript);
            for (size_t c = 0; c < chroms.size(); ++c) R.vmask[c] = std::regex_search(chroms[c].name, re) ? 1 : 0;
        } catch (const std::regex_error&) { fprintf(stderr, "Error: bad value '%s' for %s (a regular expression)\n", R.vre.c_str(), name(O_VP_PARTNERS)); return 12; }
    }
    R.vmask[v] = 0;
    size_t np = 0;
    for (uint8_t x : R.vmask) np += x;
    if (np == 0) { fprintf(stderr, "Error: %s '%s' keeps no chromosome\n", name(O_VP_PARTNERS), R.vre.c_str()); return 12; }
    R.vo.partner_mask = R.vmask.data();
    return 0;
}
// -r, and everything given in base pairs against every resolution
static int resolutions(Run& R) {
    const char* rlist = R.a.val[O_RES];
    if (!parse_res(rlist, R.res)) { fprintf(stderr, "Error: bad resolution list '%s' (1 .. 16 different positive numbers, comma separated)\n", rlist); return 12; }
    for (uint32_t r : R.res)
        for (uint32_t bp : R.ibp)
            if (bp % r != 0 || bp / r > 1024) { fprintf(stderr, "Error: %s window %u is not a multiple of resolution %u of at most 1024 bins\n", name(O_INSULATION), bp, r); return 12; }
    const struct { const int32_t* bp; Opt o[2]; } dist[2] = {{R.sbp, {O_SADDLE_MIN_DIST, O_SADDLE_MAX_DIST}}, {R.cbp, {O_SCC_MIN_DIST, O_SCC_MAX_DIST}}};
    for (const auto& d : dist)
        for (uint32_t r : R.res)
            for (int k = 0; k < 2; ++k)
                if (d.bp[k] > 0 && (uint32_t)d.bp[k] % r != 0) { fprintf(stderr, "Error: %s %d is not a multiple of resolution %u\n", name(d.o[k]), d.bp[k], r); return 12; }
    return 0;
}
// the bins of .bins.bed in order, with a value each
static int read_track(Run& R) {
    const char* fn = R.a.val[O_EIGS_TRACK];
    if (!fn) return 0;
    if (R.res.size() != 1) { fprintf(stderr, "Error: %s needs a single resolution\n", name(O_EIGS_TRACK)); return usage(R.a.me); }
    std::vector<double>& track = R.track;
    std::string txt;
    if (!read_file(fn, txt)) { fprintf(stderr, "Error: read track file failed!\n"); return 10; }
    size_t p = 0;
    const uint64_t r = R.res[0];
    for (const Chrom& c : R.chroms)
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
    return 0;
}
static int bin_limit(Run& R) {
    for (uint32_t r : R.res) {
        uint64_t nb = 0;
        for (const Chrom& c : R.chroms) nb += (c.len + r - 1) / r;
        if (nb >= (1ull << 32)) { fprintf(stderr, "Error: resolution %u gives 2^32 bins or more\n", r); return 12; }
    }
    return 0;
}
static int read_features(Run& R) {
    const char* fn = R.a.val[O_PILEUP];
    if (!fn) return 0;
    std::string txt, why;
    if (!read_file(fn, txt)) { fprintf(stderr, "Error: read pileup file failed!\n"); return 10; }
    if (!parse_bedpe(txt, R.chroms, R.anchors, why)) { fprintf(stderr, "Error: bad pileup file: %s\n", why.c_str()); return 12; }
    return 0;
}
static int open_inputs(Run& R) {
    for (const char* fn : R.a.files) {
        FILE* f = strcmp(fn, "-") ? fopen(fn, "rb") : stdin;
        if (!f) return R.fail_read();
        R.in.emplace_back(f);
    }
    if (R.in.empty()) R.in.emplace_back(stdin);
    if (R.a.on(O_COMPARE)) {
        R.in2.reset(fopen(R.a.val[O_COMPARE], "rb"));
        if (!R.in2) return R.fail_read();
    }
    return 0;
}

// ---- the device: every function returns 0 or the exit code, and calls the library in the order the parent of this file did ---------------
// every byte of f into matrix mx; a file without a final newline does not run into the next one
// A BGZF file (known by its magic bytes, not by its name) is inflated on the device (mkt_bgzf_* of include/mkt.h) and handed over
// there: the text makes no host round trip, except the part of a last line that has no newline.
struct Bgzf {                                        // owns a mkt_bgzf
    mkt_bgzf* p = nullptr;
    ~Bgzf() { if (p) mkt_bgzf_destroy(p); }
};
static int add_bgzf(Run& R, mkt_matrix* mx, File& f, bool compare, size_t k) {
    const char* e = getenv("MKT_DEVICE");
    Bgzf z;
    if (!R.ok(mkt_bgzf_create(e ? atoi(e) : 0, &z.p))) { fprintf(stderr, "Error: GPU inflate: %s\n", mkt_strerror(R.rc)); return 20; }
    auto fail = [&]() { fprintf(stderr, "Error: GPU inflate%s: %s: %s\n", compare ? " (--compare)" : "", mkt_strerror(R.rc), mkt_bgzf_error(z.p)); return R.rc == MKT_E_FORMAT ? 12 : 21; };
    for (; k > 0; k = fread(R.buf.data(), 1, R.buf.size(), f.get()))
        if (!R.ok(mkt_bgzf_add(z.p, R.buf.data(), k))) return fail();
    if (ferror(f.get())) return R.fail_read();
    f.reset();
    const void* d = nullptr;
    uint64_t n = 0;
    if (!R.ok(mkt_bgzf_run(z.p, nullptr, nullptr)) || !R.ok(mkt_bgzf_device_text(z.p, &d, &n))) return fail();
    if (!n) return 0;
    // whole lines go over on the device; what stands behind the last newline (looked for in the last MiB) goes the way of plain text
    const uint64_t w = n < ((uint64_t)1 << 20) ? n : ((uint64_t)1 << 20);
    if (!R.ok(mkt_bgzf_fetch_text(z.p, n - w, R.buf.data(), (size_t)w))) return fail();
    uint64_t t = w;
    while (t > 0 && R.buf[t - 1] != '\n') --t;
    const uint64_t whole = t ? n - w + t : 0;         // no newline in the window: everything goes through the host
    std::string tail;
    if (t) tail.assign(R.buf.data() + t, (size_t)(w - t));
    else { tail.resize((size_t)n); if (!R.ok(mkt_bgzf_fetch_text(z.p, 0, &tail[0], (size_t)n))) return fail(); }
    if (whole && !R.ok(mkt_matrix_add_device(mx, d, (size_t)whole))) return R.fail_lib("GPU matrix", compare);
    if (!tail.empty()) {
        if (!compare) tail.push_back('\n');
        if (!R.ok(mkt_matrix_add(mx, tail.data(), tail.size()))) return R.fail_lib("GPU matrix", compare);
    }
    return 0;
}
static int add_file(Run& R, mkt_matrix* mx, File& f, bool compare) {
    char last = '\n';
    for (bool first = true;; first = false) {
        const size_t k = fread(R.buf.data(), 1, R.buf.size(), f.get());
        if (k == 0) break;
        if (first && k >= 4 && (unsigned char)R.buf[0] == 0x1f && (unsigned char)R.buf[1] == 0x8b) return add_bgzf(R, mx, f, compare, k);
        last = R.buf[k - 1];
        if (!R.ok(mkt_matrix_add(mx, R.buf.data(), k))) return R.fail_lib("GPU matrix", compare);
    }
    if (ferror(f.get())) return R.fail_read();
    f.reset();
    if (!compare && last != '\n' && !R.ok(mkt_matrix_add(mx, "\n", 1))) return R.fail_lib("GPU matrix");
    return 0;
}
static int bin_inputs(Run& R) {
    const char* e = getenv("MKT_DEVICE");
    const int dev = e ? atoi(e) : 0;
    if (!R.ok(mkt_matrix_create(dev, R.ttxt.data(), R.ttxt.size(), R.res.data(), (uint32_t)R.res.size(), &R.m.p))) {
        if (R.rc == MKT_E_NO_DEVICE) { fprintf(stderr, "Error: GPU matrix: %s\n", mkt_strerror(R.rc)); return 20; }
        fprintf(stderr, "Error: GPU matrix: %s: %s\n", mkt_strerror(R.rc), mkt_matrix_error(nullptr));
        return R.rc == MKT_E_ARG || R.rc == MKT_E_CAPACITY ? 12 : 21;
    }
    R.buf.resize((size_t)64 << 20);
    for (File& f : R.in)
        if (const int rc = add_file(R, R.m, f, false)) return rc;
    if (!R.ok(mkt_matrix_run(R.m, &R.pairs, &R.skipped))) return R.fail_lib("GPU matrix");
    if (!R.a.on(O_COMPARE)) return 0;
    if (!R.ok(mkt_matrix_create(dev, R.ttxt.data(), R.ttxt.size(), R.res.data(), (uint32_t)R.res.size(), &R.m2.p))) {     // the same table and resolutions
        fprintf(stderr, "Error: GPU matrix: %s: %s\n", mkt_strerror(R.rc), mkt_matrix_error(nullptr));
        return 21;
    }
    if (const int rc = add_file(R, R.m2, R.in2, true)) return rc;
    if (!R.ok(mkt_matrix_run(R.m2, nullptr, nullptr))) return R.fail_lib("GPU matrix", true);
    return 0;
}

// two profiles: the links at the partner bin, the partner track at the track bin
static int viewpoint(Run& R) {
    static const char what[] = "GPU viewpoint profile";
    const mkt_viewpoint_opts& vo = R.vo;
    std::vector<std::string> names;
    for (const Chrom& c : R.chroms) names.push_back(c.name);
    mkt_viewpoint_info vi, ti;
    mkt_viewpoint_opts lo2 = vo;
    lo2.min_count = 1;
    if (!R.ok(mkt_matrix_viewpoint(R.m, &lo2, &vi))) return R.fail_lib(what);
    std::vector<mkt::VpLink> links(vi.links);
    std::vector<uint32_t> a(vi.links), b(vi.links), c(vi.links), d(vi.links), track(vi.viewpoint_bins);
    if (!R.ok(mkt_matrix_fetch_viewpoint_links(R.m, 0, vi.links, a.data(), b.data(), c.data(), d.data()))) return R.fail_lib(what);
    if (!R.ok(mkt_matrix_fetch_viewpoint_track(R.m, 0, vi.viewpoint_bins, track.data()))) return R.fail_lib(what);
    for (size_t k = 0; k < links.size(); ++k) links[k] = {a[k], b[k], c[k], d[k]};
    const std::string bg = mkt::vp_track_text(track, R.vname, vo.vbin), lk = mkt::vp_links_text(links, names, vi.min_loop, vo.vbin, vo.pbin);
    mkt_viewpoint_opts to = vo;
    to.pbin = (uint32_t)R.vtrack_bin;
    if (!R.ok(mkt_matrix_viewpoint(R.m, &to, &ti))) return R.fail_lib(what);
    std::vector<mkt::VpCell> cells(ti.partner_cells_kept);
    a.resize(cells.size()); b.resize(cells.size()); c.resize(cells.size());
    if (!R.ok(mkt_matrix_fetch_viewpoint_partners(R.m, 0, cells.size(), a.data(), b.data(), c.data()))) return R.fail_lib(what);
    for (size_t k = 0; k < cells.size(); ++k) cells[k] = {a[k], b[k], c[k]};
    const std::string pt = mkt::vp_partners_text(cells, names, (uint64_t)R.vtrack_bin);
    size_t np = 0;
    for (uint8_t x : R.vmask) np += x;
    std::string vs = std::string("Viewpoint\t") + R.vname + "\nPartners\t" + std::to_string(np) + "\nSecondSideOnly\t" + std::to_string(vo.second_side_only) + "\nViewpointBin\t" + std::to_string(vo.vbin) +
                     "\nPartnerBin\t" + std::to_string(vo.pbin) + "\nTrackBin\t" + std::to_string(R.vtrack_bin) + "\nMinCount\t" + std::to_string(vo.min_count) + "\nHotspotRatio\t";
    put_num(vs, vo.hotspot_ratio);
    vs += "\nTotal\t" + std::to_string(vi.total) + "\nLinks\t" + std::to_string(vi.links) + "\nMinLoop\t" + std::to_string(vi.min_loop) + "\nLinksKept\t" + std::to_string(vi.links_kept) +
          "\nViewpointBins\t" + std::to_string(vi.viewpoint_bins) + "\nPartnerCells\t" + std::to_string(ti.partner_cells) + "\nPartnerCellsKept\t" + std::to_string(ti.partner_cells_kept) +
          "\nSkipped\t" + std::to_string(R.skipped) + "\n";                    // pairs the matrix stage left out: they are absent from the profile
    if (!write_file(R.pre + ".viewpoint.bedgraph", bg.data(), bg.size()) || !write_file(R.pre + ".viewpoint.links", lk.data(), lk.size()) ||
        !write_file(R.pre + ".partners.bedgraph", pt.data(), pt.size()) || !write_file(R.pre + ".viewpoint.stat", vs.data(), vs.size())) return R.fail_write();
    return 0;
}

// the size of the resolution, its line of the .stat, its first bins, and <prefix>.<r>.coo as the device made it
static int begin_level(Run& R, Level& L, uint32_t k) {
    uint64_t nnz = 0, tb = 0, nb = 0;
    L.k = k; L.r = R.res[k]; L.base = R.pre + "." + std::to_string(L.r);
    L.first.clear();
    for (const Chrom& c : R.chroms) { L.first.push_back(nb); nb += (c.len + L.r - 1) / L.r; }
    if (!R.ok(mkt_matrix_info(R.m, k, &L.nbins, &nnz, &tb))) return R.fail_lib("GPU matrix");
    R.stat += "nnz." + std::to_string(L.r) + "\t" + std::to_string(nnz) + "\n";
    File f(fopen((L.base + ".coo").c_str(), "wb"));
    if (!f) return R.fail_write();
    for (uint64_t off = 0; off < tb; off += R.buf.size()) {
        const size_t n = tb - off < R.buf.size() ? (size_t)(tb - off) : R.buf.size();
        if (!R.ok(mkt_matrix_fetch_text(R.m, k, off, R.buf.data(), n))) return R.fail_lib("GPU matrix");
        if (fwrite(R.buf.data(), 1, n, f.get()) != n) return R.fail_write();
    }
    return fclose(f.release()) != 0 ? R.fail_write() : 0;
}
static int balance(Run& R, const Level& L) {
    mkt_balance_stats bs;
    if (!R.ok(mkt_matrix_balance(R.m, L.k, &R.bo, &bs))) return R.fail_lib("GPU matrix balance");
    R.weights.resize(L.nbins);
    if (!R.ok(mkt_matrix_fetch_weights(R.m, L.k, 0, L.nbins, R.weights.data()))) return R.fail_lib("GPU matrix balance");
    char line[160];
    snprintf(line, sizeof line, "%u\t%u\t%d\t%.17g\t%.17g\t%llu\n", L.r, bs.iterations, bs.converged, bs.var, bs.scale, (unsigned long long)bs.masked);
    R.bstat += line;
    if (!bs.converged) fprintf(stderr, "WARN: balancing at resolution %u did not converge in %u iterations (var %g).\n", L.r, bs.iterations, bs.var);
    return 0;
}
// the replicate balanced with the same options, the strata table as <prefix>.<r>.scc.tsv and the per-chromosome scores as rows of the .stat
static int scc(Run& R, const Level& L) {
    static const char what[] = "GPU matrix scc";
    mkt_scc_opts& co = R.co;
    if (R.a.on(O_BALANCE) && !R.ok(mkt_matrix_balance(R.m2, L.k, &R.bo, nullptr))) return R.fail_lib("GPU matrix balance", true);
    co.min_diag = R.cbp[0] > 0 ? R.cbp[0] / (int32_t)L.r : 0;
    if (R.cbp[1] >= 0) co.max_diag = R.cbp[1] / (int32_t)L.r;
    else { co.max_diag = (int32_t)(5000000u / L.r); if (co.max_diag < 1) co.max_diag = 1; if (co.max_diag < co.min_diag) co.max_diag = co.min_diag; }
    mkt_scc_info ci;
    if (!R.ok(mkt_matrix_scc(R.m, L.k, R.m2, L.k, &co, &ci))) return R.fail_lib(what);
    const size_t D = ci.strata, rows = (size_t)ci.n_chrom * D;
    std::vector<uint64_t> nc(rows), nu(rows), sc(ci.n_chrom);
    std::vector<double> v[7], cs(ci.n_chrom), cn(ci.n_chrom), cd(ci.n_chrom);
    for (auto& x : v) x.resize(rows);
    if (!R.ok(mkt_matrix_fetch_scc_strata(R.m, L.k, 0, rows, nc.data(), nu.data(), v[0].data(), v[1].data(), v[2].data(), v[3].data(), v[4].data(), v[5].data(), v[6].data()))) return R.fail_lib(what);
    if (!R.ok(mkt_matrix_fetch_scc_chrom(R.m, L.k, 0, ci.n_chrom, cs.data(), cn.data(), cd.data(), sc.data()))) return R.fail_lib(what);
    ChunkedFile f(L.base + ".scc.tsv");
    std::string& t = f.text();
    t = "chrom\tdiag\tdist_bp\tn_cand\tn\tsx\tsy\tsxx\tsyy\tsxy\trho\tw\n";
    for (size_t c = 0; c < ci.n_chrom; ++c)
        for (size_t j = 0; j < D; ++j) {
            const size_t at = c * D + j;
            const uint64_t d = (uint64_t)co.min_diag + j;
            t += R.chroms[c].name; t += '\t'; t += std::to_string(d); t += '\t'; t += std::to_string(d * L.r); t += '\t'; t += std::to_string(nc[at]); t += '\t'; t += std::to_string(nu[at]);
            for (auto& x : v) { t += '\t'; put_num(t, x[at]); }
            t += '\n';
            f.wrote();
        }
    if (!f.finish()) return R.fail_write();
    std::string& stat = R.cstat;
    const std::string rs = std::to_string(L.r);
    for (size_t c = 0; c < ci.n_chrom; ++c) {
        stat += rs; stat += "\tchrom\t"; stat += R.chroms[c].name; stat += '\t'; stat += std::to_string(sc[c]); stat += '\t'; put_num(stat, cn[c]); stat += '\t'; put_num(stat, cd[c]);
        stat += '\t'; put_num(stat, cs[c]); stat += '\n';
    }
    stat += rs; stat += "\tgenome";
    for (uint64_t x : {(uint64_t)ci.n_chrom, (uint64_t)ci.strata, ci.candidates, ci.used, ci.scored, ci.count_a, ci.count_b}) { stat += '\t'; stat += std::to_string(x); }
    stat += '\t'; put_num(stat, ci.scc); stat += '\n';
    return 0;
}
// the three tables of the expected values
static int expected(Run& R, const Level& L) {
    static const char what[] = "GPU matrix expected";
    mkt_expected_opts eo;
    mkt_expected_opts_default(&eo);
    eo.use_weights = R.a.on(O_BALANCE) ? 1 : 0;
    mkt_expected_info ei;
    if (!R.ok(mkt_matrix_expected(R.m, L.k, &eo, &ei))) return R.fail_lib(what);
    std::vector<uint64_t> nv, cs;
    std::vector<double> bs, ex, sm;
    auto size = [&](uint64_t rows) { nv.resize(rows); cs.resize(rows); bs.resize(rows); ex.resize(rows); sm.resize(rows); };
    size(ei.genome_rows);
    if (!R.ok(mkt_matrix_fetch_expected_genome(R.m, L.k, 0, ei.genome_rows, nv.data(), cs.data(), bs.data(), ex.data(), sm.data()))) return R.fail_lib(what);
    ChunkedFile fg(L.base + ".expected.tsv"), fc(L.base + ".expected.chrom.tsv"), ft(L.base + ".expected.trans.tsv");
    fg.text() = "diag\tdist_bp\tn_valid\tcount_sum\tbalanced_sum\texpected\texpected_smooth\n";
    for (uint64_t d = 0; d < ei.genome_rows; ++d) {
        std::string& t = fg.text();
        t += std::to_string(d); t += '\t'; t += std::to_string(d * L.r); t += '\t'; t += std::to_string(nv[d]); t += '\t'; t += std::to_string(cs[d]); t += '\t';
        put_num(t, bs[d]); t += '\t'; put_num(t, ex[d]); t += '\t'; put_num(t, sm[d]); t += '\n';
        fg.wrote();
    }
    const bool okg = fg.finish();
    size(ei.cis_rows);
    if (!R.ok(mkt_matrix_fetch_expected_cis(R.m, L.k, 0, ei.cis_rows, nv.data(), cs.data(), bs.data()))) return R.fail_lib(what);
    fc.text() = "chrom\tdiag\tn_valid\tcount_sum\tbalanced_sum\n";
    uint64_t row = 0;
    for (const Chrom& c : R.chroms)
        for (uint64_t d = 0, n = (c.len + L.r - 1) / L.r; d < n; ++d, ++row) {
            std::string& t = fc.text();
            t += c.name; t += '\t'; t += std::to_string(d); t += '\t'; t += std::to_string(nv[row]); t += '\t'; t += std::to_string(cs[row]); t += '\t';
            put_num(t, bs[row]); t += '\n';
            fc.wrote();
        }
    const bool okc = okg && fc.finish();
    size(ei.trans_rows);
    if (!R.ok(mkt_matrix_fetch_expected_trans(R.m, L.k, 0, ei.trans_rows, nv.data(), cs.data(), bs.data(), ex.data()))) return R.fail_lib(what);
    ft.text() = "chrom1\tchrom2\tn_valid\tcount_sum\tbalanced_sum\texpected\n";
    row = 0;
    for (size_t a = 0; a < R.chroms.size(); ++a)
        for (size_t b = a + 1; b < R.chroms.size(); ++b, ++row) {
            std::string& t = ft.text();
            t += R.chroms[a].name; t += '\t'; t += R.chroms[b].name; t += '\t'; t += std::to_string(nv[row]); t += '\t'; t += std::to_string(cs[row]); t += '\t';
            put_num(t, bs[row]); t += '\t'; put_num(t, ex[row]); t += '\n';
            ft.wrote();
        }
    return okc && ft.finish() ? 0 : R.fail_write();
}
// a pileup around the cells (pa, pb): the arrays as <prefix>.<r>.<ext> and one more row of `stat`
static int pileup_of(Run& R, const Level& L, const std::vector<uint32_t>& pa, const std::vector<uint32_t>& pb, const char* ext, std::string& stat) {
    static const char what[] = "GPU matrix pileup";
    mkt_pileup_info pi;
    if (!R.ok(mkt_matrix_pileup(R.m, L.k, pa.data(), pb.data(), pa.size(), &R.po, &pi))) return R.fail_lib(what);
    const size_t S = pi.side, S2 = S * S;
    std::vector<uint64_t> n(S2), cs(S2);
    std::vector<double> vs(S2), mean(S2);
    if (!R.ok(mkt_matrix_fetch_pileup(R.m, L.k, n.data(), cs.data(), vs.data(), mean.data()))) return R.fail_lib(what);
    std::string t = "p\tq\tn\tcsum\tvsum\tmean\n";
    const int flank = (int)(S / 2);
    for (size_t x = 0; x < S2; ++x) {
        t += std::to_string((int)(x / S) - flank); t += '\t'; t += std::to_string((int)(x % S) - flank); t += '\t'; t += std::to_string(n[x]); t += '\t'; t += std::to_string(cs[x]); t += '\t';
        put_num(t, vs[x]); t += '\t'; put_num(t, mean[x]); t += '\n';
    }
    if (!write_file(L.base + ext, t.data(), t.size())) return R.fail_write();
    stat += std::to_string(L.r);
    for (uint64_t v : {pi.features, pi.used, pi.trans, pi.edge, pi.dist}) { stat += '\t'; stat += std::to_string(v); }
    for (double v : {pi.peak, pi.p2ll, pi.p2ul, pi.p2ur, pi.p2lr, pi.p2m, pi.z_ll}) { stat += '\t'; put_num(stat, v); }
    stat += '\n';
    return 0;
}
// <prefix>.<r>.loops.bedpe and, with --apa, the pileup around the peak cells in loop order
static int loops(Run& R, const Level& L) {
    static const char what[] = "GPU matrix loops";
    mkt_loops_info li;
    if (!R.ok(mkt_matrix_loops(R.m, L.k, &R.lo, &li))) return R.fail_lib(what);
    std::vector<mkt_loop> rows(li.loops);
    if (!R.ok(mkt_matrix_fetch_loops(R.m, L.k, 0, li.loops, rows.data()))) return R.fail_lib(what);
    R.lstat += std::to_string(L.r);
    for (uint64_t v : {li.cells, li.candidates, li.tested, li.undefined, li.over, li.grew, li.at_max, li.enriched, li.loops}) { R.lstat += '\t'; R.lstat += std::to_string(v); }
    R.lstat += '\n';
    std::string t = "#chrom1\tstart1\tend1\tchrom2\tstart2\tend2\tcount\texpected_donut\texpected_ll\texpected_h\texpected_v\twindow\tcells\tbox_start1\tbox_end1\tbox_start2\tbox_end2\n";
    std::vector<uint32_t> pa, pb;
    for (const mkt_loop& l : rows) {
        const size_t c = chrom_of(L, l.bin1);
        const std::string& nm = R.chroms[c].name;
        t += nm; t += '\t'; span(t, R, L, c, l.bin1, l.bin1); t += '\t'; t += nm; t += '\t'; span(t, R, L, c, l.bin2, l.bin2); t += '\t';
        t += std::to_string(l.count);
        for (int q = 0; q < 4; ++q) { t += '\t'; put_num(t, l.r[q]); }
        t += '\t'; t += std::to_string(l.window); t += '\t'; t += std::to_string(l.n_cells); t += '\t';
        span(t, R, L, c, l.box[0], l.box[1]); t += '\t'; span(t, R, L, c, l.box[2], l.box[3]); t += '\n';
        pa.push_back(l.bin1); pb.push_back(l.bin2);
    }
    if (!write_file(L.base + ".loops.bedpe", t.data(), t.size())) return R.fail_write();
    return R.a.on(O_APA) ? pileup_of(R, L, pa, pb, ".apa.tsv", R.astat) : 0;
}
// the pileup around the features of the file: an anchor's bin is that of its midpoint, the smaller bin first
static int pileup(Run& R, const Level& L) {
    std::vector<uint32_t> pa, pb;
    for (const Anchor& a : R.anchors) {
        const uint32_t x = (uint32_t)(L.first[a.c1] + a.m1 / L.r), y = (uint32_t)(L.first[a.c2] + a.m2 / L.r);
        pa.push_back(x < y ? x : y); pb.push_back(x < y ? y : x);
    }
    return pileup_of(R, L, pa, pb, ".pileup.tsv", R.pstat);
}
// the tables, the group edges and the profile of the saddle with eigenvector 1 as the track: <prefix>.<r>.saddle.tsv and rows of the .stat
static int saddle(Run& R, const Level& L) {
    static const char what[] = "GPU matrix saddle";
    mkt_saddle_opts& so = R.so;
    if (R.sbp[0] >= 0) so.min_diag = R.sbp[0] / (int32_t)L.r;
    if (R.sbp[1] >= 0) so.max_diag = R.sbp[1] / (int32_t)L.r;
    mkt_saddle_info si;
    if (!R.ok(mkt_matrix_saddle(R.m, L.k, &so, R.evec.data(), &si))) return R.fail_lib(what);
    const size_t Q = si.n_groups, Q2 = Q * Q;
    std::vector<uint64_t> n(Q2), nz(Q2), cs(Q2), gb(Q);
    std::vector<double> vs(Q2), mean(Q2), lo(Q), hi(Q), st(Q / 2), aa(Q / 2), bb(Q / 2);
    if (!R.ok(mkt_matrix_fetch_saddle(R.m, L.k, n.data(), nz.data(), cs.data(), vs.data(), mean.data()))) return R.fail_lib(what);
    if (!R.ok(mkt_matrix_fetch_saddle_edges(R.m, L.k, gb.data(), lo.data(), hi.data()))) return R.fail_lib(what);
    if (!R.ok(mkt_matrix_fetch_saddle_profile(R.m, L.k, st.data(), aa.data(), bb.data()))) return R.fail_lib(what);
    std::string t = "a\tb\tn\tnnz\tcsum\tvsum\tmean\n";
    for (size_t a = 0; a < Q; ++a)
        for (size_t b = a; b < Q; ++b) {
            const size_t x = a * Q + b;
            t += std::to_string(a); t += '\t'; t += std::to_string(b); t += '\t'; t += std::to_string(n[x]); t += '\t'; t += std::to_string(nz[x]); t += '\t';
            t += std::to_string(cs[x]); t += '\t'; put_num(t, vs[x]); t += '\t'; put_num(t, mean[x]); t += '\n';
        }
    if (!write_file(L.base + ".saddle.tsv", t.data(), t.size())) return R.fail_write();
    std::string& stat = R.sstat;
    const std::string rs = std::to_string(L.r);
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
    return 0;
}
// the eigenvectors for the per-bin file, a row of the .stat per chromosome and, with --saddle, the saddle of the first vector
static int eigs(Run& R, const Level& L) {
    static const char what[] = "GPU matrix eigs";
    mkt_eigs_info gi;
    if (!R.ok(mkt_matrix_eigs(R.m, L.k, &R.go, R.track.empty() ? nullptr : R.track.data(), &gi))) return R.fail_lib(what);
    const uint32_t ne = R.ne = (uint32_t)R.go.n_eigs;
    R.evec.resize((size_t)ne * L.nbins);
    for (uint32_t j = 0; j < ne; ++j)
        if (!R.ok(mkt_matrix_fetch_eigvecs(R.m, L.k, j, 0, L.nbins, R.evec.data() + (size_t)j * L.nbins))) return R.fail_lib(what);
    std::vector<double> lam((size_t)gi.n_chrom * ne);
    std::vector<uint32_t> ng(gi.n_chrom), it(gi.n_chrom);
    std::vector<uint8_t> cv(gi.n_chrom);
    if (!R.ok(mkt_matrix_fetch_eigvals(R.m, L.k, 0, gi.n_chrom, lam.data(), nullptr, ng.data(), it.data(), cv.data()))) return R.fail_lib(what);
    std::string& gstat = R.gstat;
    for (uint32_t c = 0; c < gi.n_chrom; ++c) {
        const Chrom& ch = R.chroms[c];
        gstat += std::to_string(L.r); gstat += '\t'; gstat += ch.name; gstat += '\t'; gstat += std::to_string((ch.len + L.r - 1) / L.r);
        gstat += '\t'; gstat += std::to_string(ng[c]); gstat += '\t'; gstat += std::to_string(it[c]); gstat += '\t'; gstat += cv[c] ? '1' : '0';
        for (uint32_t j = 0; j < ne; ++j) { gstat += '\t'; put_num(gstat, lam[(size_t)c * ne + j]); }
        gstat += '\n';
        if (it[c] && !cv[c]) fprintf(stderr, "WARN: eigenvectors of %s at resolution %u did not converge in %u iterations.\n", ch.name.c_str(), L.r, it[c]);
    }
    return R.a.on(O_SADDLE) ? saddle(R, L) : 0;
}
// the scores of every window for the per-bin file and a row of the .stat per window
static int insulation(Run& R, const Level& L) {
    static const char what[] = "GPU matrix insulation";
    const uint32_t ni = (uint32_t)R.ibp.size();
    const uint64_t nbins = L.nbins;
    R.io.n_windows = (int32_t)ni;
    for (uint32_t j = 0; j < 4; ++j) R.io.window[j] = j < ni ? (int32_t)(R.ibp[j] / L.r) : 0;
    mkt_insulation_info ii;
    if (!R.ok(mkt_matrix_insulation(R.m, L.k, &R.io, &ii))) return R.fail_lib(what);
    R.inv.resize((size_t)ni * nbins); R.isc.resize((size_t)ni * nbins); R.ilg.resize((size_t)ni * nbins); R.ist.resize((size_t)ni * nbins); R.ibd.resize((size_t)ni * nbins);
    for (uint32_t j = 0; j < ni; ++j) {
        const size_t at = (size_t)j * nbins;
        if (!R.ok(mkt_matrix_fetch_insulation(R.m, L.k, j, 0, nbins, R.inv.data() + at, nullptr, nullptr, R.isc.data() + at, R.ilg.data() + at, R.ist.data() + at, R.ibd.data() + at)))
            return R.fail_lib(what);
        R.istat += std::to_string(L.r); R.istat += '\t'; R.istat += std::to_string(R.ibp[j]); R.istat += '\t'; R.istat += std::to_string(nbins);
        for (uint64_t v : {ii.defined[j], ii.minima[j], ii.boundaries[j]}) { R.istat += '\t'; R.istat += std::to_string(v); }
        R.istat += '\n';
    }
    return 0;
}
// <prefix>.<r>.bins.bed and, with the same three columns in front, the weights, the eigenvectors and the insulation scores of every bin
static int per_bin_files(Run& R, const Level& L) {
    const bool with_w = R.a.on(O_BALANCE), with_e = R.a.on(O_EIGS);
    const uint32_t ni = (uint32_t)R.ibp.size(), ne = R.ne;
    const uint64_t r = L.r, nbins = L.nbins;
    ChunkedFile bed(L.base + ".bins.bed"), wbed(L.base + ".weights.bed"), gbed(L.base + ".eigs.tsv"), ibed(L.base + ".insulation.tsv");
    if (ni) {
        std::string& t = ibed.text();
        t = "chrom\tstart\tend";
        for (uint32_t j = 0; j < ni; ++j)
            for (const char* col : {"n_valid_", "score_", "log2_insulation_score_", "boundary_strength_", "is_boundary_"}) { t += '\t'; t += col; t += std::to_string(R.ibp[j]); }
        t += '\n';
    }
    if (with_e) { std::string& t = gbed.text(); t = "chrom\tstart\tend"; for (uint32_t j = 0; j < ne; ++j) { t += "\tE"; t += std::to_string(j + 1); } t += '\n'; }
    uint64_t bin = 0;
    std::string at;                                                          // chrom \t start \t end of the bin at hand
    for (const Chrom& c : R.chroms)
        for (uint64_t s = 0; s < c.len; s += r, ++bin) {
            at = c.name; at += '\t'; at += std::to_string(s); at += '\t'; at += std::to_string(s + r < c.len ? s + r : c.len);
            bed.text() += at; bed.text() += '\n';
            bed.wrote();
            if (with_w) { std::string& t = wbed.text(); t += at; t += '\t'; put_num(t, R.weights[bin]); t += '\n'; wbed.wrote(); }
            if (with_e) {
                std::string& t = gbed.text();
                t += at;
                for (uint32_t j = 0; j < ne; ++j) { t += '\t'; put_num(t, R.evec[(size_t)j * nbins + bin]); }
                t += '\n';
                gbed.wrote();
            }
            if (ni) {
                std::string& t = ibed.text();
                t += at;
                for (uint32_t j = 0; j < ni; ++j) {
                    const size_t x = (size_t)j * nbins + bin;
                    t += '\t'; t += std::to_string(R.inv[x]); t += '\t'; put_num(t, R.isc[x]); t += '\t'; put_num(t, R.ilg[x]); t += '\t'; put_num(t, R.ist[x]);
                    t += R.ibd[x] ? "\t1" : "\t0";
                }
                t += '\n';
                ibed.wrote();
            }
        }
    return bed.finish() && (!with_w || wbed.finish()) && (!with_e || gbed.finish()) && (!ni || ibed.finish()) ? 0 : R.fail_write();
}
// every resolution in one container, with the weights of --balance
static int hic(Run& R) {
    static const char what[] = "GPU .hic container";
    mkt_hic_info hi;
    if (!R.ok(mkt_matrix_hic(R.m, &R.ho, &hi))) return R.fail_lib(what);
    ChunkedFile f(R.pre + ".hic");
    for (uint64_t off = 0; off < hi.file_bytes; off += R.buf.size()) {
        const size_t n = (size_t)std::min<uint64_t>(R.buf.size(), hi.file_bytes - off);
        if (!R.ok(mkt_matrix_fetch_hic(R.m, off, R.buf.data(), n))) return R.fail_lib(what);
        if (!f.append(R.buf.data(), n)) return R.fail_write();
    }
    const std::string hs = "FileBytes\t" + std::to_string(hi.file_bytes) + "\nMatrices\t" + std::to_string(hi.matrices) + "\nBlocks\t" + std::to_string(hi.blocks) +
                           "\nFloatBlocks\t" + std::to_string(hi.float_blocks) + "\nPieces\t" + std::to_string(hi.pieces) + "\nRawBytes\t" + std::to_string(hi.raw_bytes) +
                           "\nDeflatedBytes\t" + std::to_string(hi.deflated_bytes) + "\nLevel\t" + std::to_string(R.ho.level) + "\nBlockBins\t" + std::to_string(R.ho.block_bins) + "\n";
    return f.finish() && write_file(R.pre + ".hic.stat", hs.data(), hs.size()) ? 0 : R.fail_write();
}
static int write_stats(Run& R) {
    const struct { bool on; const char* ext; const std::string& text; } files[] = {
        {R.a.on(O_COMPARE), ".scc.stat", R.cstat}, {R.a.on(O_SADDLE), ".saddle.stat", R.sstat}, {R.a.on(O_APA), ".apa.stat", R.astat}, {R.a.on(O_PILEUP), ".pileup.stat", R.pstat},
        {!R.ibp.empty(), ".insulation.stat", R.istat}, {R.a.on(O_EIGS), ".eigs.stat", R.gstat}, {R.a.on(O_BALANCE), ".balance.stat", R.bstat}, {R.a.on(O_LOOPS), ".loops.stat", R.lstat},
        {true, ".matrix.stat", R.stat}};
    for (const auto& f : files)
        if (f.on && !write_file(R.pre + f.ext, f.text.data(), f.text.size())) return R.fail_write();
    return 0;
}

int main(int argc, char* argv[]) {
    Run R;
    const Args& a = R.a;
    int rc;
    if ((rc = scan(argc, argv, R.a))) return rc;
    // the order of these checks is the order errors are reported in: tests/golden/pairs2matrix_cli_golden.json holds it
    for (int (*check)(Run&) : {hic_options, balance_options, loops_options, eigs_options, insulation_options, pileup_options, saddle_options, scc_options, viewpoint_options,
                               insulation_windows, read_table, viewpoint_partners, resolutions, read_track, bin_limit, read_features, open_inputs})
        if ((rc = check(R))) return rc;
    R.pre = a.val[O_PREFIX];
    if ((rc = bin_inputs(R))) return rc;
    if (R.vname && (rc = viewpoint(R))) return rc;
    R.stat = "Pairs\t" + std::to_string(R.pairs) + "\nBinned\t" + std::to_string(R.pairs - R.skipped) + "\nSkipped\t" + std::to_string(R.skipped) + "\n";
    Level L;
    for (uint32_t k = 0; k < R.res.size(); ++k) {                            // results in the library invalidate each other: this order is fixed
        if ((rc = begin_level(R, L, k))) return rc;
        if (a.on(O_BALANCE) && (rc = balance(R, L))) return rc;
        if (a.on(O_COMPARE) && (rc = scc(R, L))) return rc;
        if (a.on(O_EXPECTED) && (rc = expected(R, L))) return rc;
        if (a.on(O_LOOPS) && (rc = loops(R, L))) return rc;
        if (a.on(O_PILEUP) && (rc = pileup(R, L))) return rc;
        if (a.on(O_EIGS) && (rc = eigs(R, L))) return rc;
        if (!R.ibp.empty() && (rc = insulation(R, L))) return rc;
        if ((rc = per_bin_files(R, L))) return rc;
    }
    if (a.on(O_HIC) && (rc = hic(R))) return rc;
    return write_stats(R);
}
