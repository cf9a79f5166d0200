// mkt_trim.h -- the host half of adapter and quality trimming (mkt_trim.hip): the argument check, the built-in adapter table, the table
// "compared length -> allowed mismatches" that carries the one float32 decision of the definition (include/mkt.h, "adapter and quality
// trimming") into the kernels' integer arithmetic, and the validation of a record's shape.  No HIP in here.
#pragma once
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>
#include "../../include/mkt.h"

#ifdef __HIPCC__
#define MKT_TRIM_HD __host__ __device__
#else
#define MKT_TRIM_HD
#endif

namespace mkt {

constexpr uint32_t TR_SEED = 3;                               // letters of an adapter's head that seed a candidate
constexpr uint32_t TR_DIMER = 1;                              // an adapter at cycle 0 or 1: a dimer
enum { TR_PASS = 0, TR_DROP_QUALITY = 1, TR_ADAPTER = 2, TR_TAILHIT = 3 };
enum { TR_BAD_HEADER = 1, TR_BAD_PLUS = 2, TR_BAD_LONG_HEADER = 3, TR_BAD_LONG = 4, TR_BAD_QLEN = 5, TR_BAD_QUAL = 6 };

struct TrParams {                                             // passed to the kernels by value
    uint32_t min_size, phred, thr /* phred + min_qual */, window, alen;
    uint8_t a1[MKT_TRIM_MAX_ADAPTER], a2[MKT_TRIM_MAX_ADAPTER];
    uint8_t limit[MKT_TRIM_MAX_ADAPTER + 1];                  // limit[L]: mismatches allowed over L compared letters
};

struct TrKit { const char* name; const char* a1; const char* a2; };
// the names as the program spells them; CLIP is known and refused (trim_resolve)
static const TrKit kTrKits[] = {
    {"illumina", "AGATCGGAAGAGC", "AGATCGGAAGAGC"}, {"ILLUMINA", "AGATCGGAAGAGC", "AGATCGGAAGAGC"}, {"Illumina", "AGATCGGAAGAGC", "AGATCGGAAGAGC"},
    {"Nextera", "CTGTCTCTTATACACATCT", "CTGTCTCTTATACACATCT"}, {"nextera", "CTGTCTCTTATACACATCT", "CTGTCTCTTATACACATCT"},
    {"Transposase", "TCGTCGGCAGCGTC", "GTCTCGTGGGCTCG"}, {"transposase", "TCGTCGGCAGCGTC", "GTCTCGTGGGCTCG"},
    {"BGI", "AAGTCGGAGGCCAAGCGGTC", "AAGTCGGATCGTAGCCATGT"}, {"bgi", "AAGTCGGAGGCCAAGCGGTC", "AAGTCGGATCGTAGCCATGT"},
};

// limit[L], L = 0 .. MKT_TRIM_MAX_ADAPTER: ceil(float32(L) * float32(mismatch)), product and ceiling in float32
inline void trim_limits(double mismatch, uint8_t limit[MKT_TRIM_MAX_ADAPTER + 1]) {
    const volatile float m = (float)mismatch;
    for (uint32_t L = 0; L <= MKT_TRIM_MAX_ADAPTER; ++L) {
        const volatile float p = (float)L * m;
        const float c = ceilf(p);
        limit[L] = (uint8_t)(c < 0.f ? 0.f : (c > (float)L ? (float)L : c));
    }
}

// The argument check: MKT_OK and *P filled (P may be null), or MKT_E_ARG with the reason in msg.
inline int trim_resolve(const mkt_trim_opts* o, TrParams* P, char* msg, size_t cap) {
    if (msg && cap) msg[0] = 0;
    auto say = [&](const char* fmt, unsigned long long a, unsigned long long b) { if (msg && cap) snprintf(msg, cap, fmt, a, b); return (int)MKT_E_ARG; };
    if (!o) return say("no options", 0, 0);
    const char *a1 = nullptr, *a2 = nullptr;
    if (o->kit) {                                             // the kit wins over adapter1 / adapter2
        if (!strcmp(o->kit, "CLIP") || !strcmp(o->kit, "clip")) return say("the CLIP kit is not supported", 0, 0);
        for (const TrKit& k : kTrKits) if (!strcmp(o->kit, k.name)) { a1 = k.a1; a2 = k.a2; }
        if (!a1) { if (msg && cap) snprintf(msg, cap, "unknown kit '%.40s': illumina, nextera, transposase or bgi", o->kit); return (int)MKT_E_ARG; }
    } else if (!o->adapter1) {
        if (o->adapter2) return say("adapter2 is set while adapter1 is not", 0, 0);
        a1 = kTrKits[0].a1; a2 = kTrKits[0].a2;
    } else {
        a1 = o->adapter1; a2 = o->adapter2 ? o->adapter2 : o->adapter1;
    }
    size_t n = 0;                                             // the common length is what is compared
    while (a1[n] && a2[n] && n <= MKT_TRIM_MAX_ADAPTER) ++n;
    if (n < MKT_TRIM_MIN_ADAPTER || n > MKT_TRIM_MAX_ADAPTER) return say("adapter size %llu: need 8 .. %llu", n, MKT_TRIM_MAX_ADAPTER);
    for (size_t j = 0; j < n; ++j) if (a1[j] == '\n' || a1[j] == '\r' || a2[j] == '\n' || a2[j] == '\r') return say("adapter with a line end in it", 0, 0);
    if (o->min_size < 10 || o->min_size > MKT_TRIM_MAX_READ) return say("min size %llu: need 10 .. %llu", o->min_size, MKT_TRIM_MAX_READ);
    if (o->phred < 1 || o->phred > 126 || o->min_qual < 1 || o->min_qual > 126 || o->phred + o->min_qual > 126)
        return say("phred %llu / min quality %llu: need 1 .. 126 each and a sum of at most 126", o->phred, o->min_qual);
    if (o->window < 1 || o->window > MKT_TRIM_MAX_READ) return say("window %llu: need 1 .. %llu", o->window, MKT_TRIM_MAX_READ);
    if (!(o->mismatch >= 0.0 && o->mismatch <= 1.0)) { if (msg && cap) snprintf(msg, cap, "mismatch %g: need 0 .. 1", o->mismatch); return (int)MKT_E_ARG; }
    if (P) {
        memset(P, 0, sizeof *P);
        P->min_size = o->min_size; P->phred = o->phred; P->thr = o->phred + o->min_qual; P->window = o->window; P->alen = (uint32_t)n;
        memcpy(P->a1, a1, n); memcpy(P->a2, a2, n);
        trim_limits(o->mismatch, P->limit);
    }
    return MKT_OK;
}

// The shape of one record: 0, or TR_BAD_*.  h / p: first byte of the header and of the third line (0 when the line is empty).
MKT_TRIM_HD inline uint32_t trim_record_shape(uint8_t h, uint32_t header_len, uint8_t p, uint32_t seq_len, uint32_t qual_len) {
    if (h != '@') return TR_BAD_HEADER;
    if (p != '+') return TR_BAD_PLUS;
    if (header_len > MKT_TRIM_MAX_HEADER) return TR_BAD_LONG_HEADER;
    if (seq_len > MKT_TRIM_MAX_READ) return TR_BAD_LONG;
    if (seq_len != qual_len) return TR_BAD_QLEN;
    return 0;
}
MKT_TRIM_HD inline bool trim_qual_ok(uint8_t c, uint32_t phred) { return c >= phred && c <= 126u; }
MKT_TRIM_HD inline bool trim_revcomp(uint8_t x, uint8_t y) { return (x == 'A' && y == 'T') || (x == 'C' && y == 'G') || (x == 'G' && y == 'C') || (x == 'T' && y == 'A'); }

// The tail rule on k >= 10 kept cycles: the cycles kept after it (k: no tail hit).
MKT_TRIM_HD inline uint32_t trim_tail(const uint8_t* r1, const uint8_t* r2, uint32_t k, const uint8_t* a1, const uint8_t* a2) {
    uint32_t i = k - 2;
    uint32_t bad = (r1[i] != a1[0]) + (r1[i + 1] != a1[1]) + (r2[i] != a2[0]) + (r2[i + 1] != a2[1]) + !trim_revcomp(r1[5], r2[i - 6]) + !trim_revcomp(r2[5], r1[i - 6]);
    if (bad <= 1) return i;
    i = k - 1;
    bad = (r1[i] != a1[0]) + (r2[i] != a2[0]) + !trim_revcomp(r1[5], r2[i - 6]) + !trim_revcomp(r2[5], r1[i - 6]) + !trim_revcomp(r1[6], r2[i - 7]) + !trim_revcomp(r2[6], r1[i - 7]);
    return bad <= 1 ? i : k;
}

static const char* const kTrBad[] = {"", "a record that does not start with '@'", "a record whose third line does not start with '+'",
                                     "a header line longer than MKT_TRIM_MAX_HEADER (126) bytes", "a read longer than MKT_TRIM_MAX_READ (510) bases",
                                     "sequence and quality differ in length", "a quality byte outside phred .. 126"};

}  // namespace mkt
