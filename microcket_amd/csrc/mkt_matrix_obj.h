// mkt_matrix_obj.h -- the matrix object as the files that serve its entry points see it: host side, internal, not installed.  The records
// the binning kernels of mkt_matrix.hip read, one resolution's results with their lifetimes and the one function that ends them, and the
// guards an entry point starts with.  Each analysis serves its own entry points from its own .hip on top of this.  DESIGN.md 7a.
#pragma once
#include <hip/hip_runtime.h>
#include <stdarg.h>
#include <stdio.h>
#include <string.h>
#include <string>
#include <unordered_map>
#include <vector>

#include "../../include/mkt.h"
#include "mkt_core.h"
#include "mkt_chromtab.h"
#include "mkt_layout.h"
#include "mkt_balance.h"
#include "mkt_expected.h"
#include "mkt_loops.h"
#include "mkt_eigs.h"
#include "mkt_insulation.h"
#include "mkt_pileup.h"
#include "mkt_saddle.h"
#include "mkt_scc.h"
#include "mkt_viewpoint.h"
#include "mkt_hic.h"

namespace mkt {

// MX_SKIP (MxRec::ia of a skipped pair), the given table MxTab and its lookup: mkt_chromtab.h
constexpr uint32_t MX_NONE = 0xFFFFFFFEu;          // MxRec::ia of something that is not a pair (a '#' line, a pair left out by its flag)
struct MxRec { uint32_t ia, pa, ib, pb; };         // table index and 1-based position of the two sides
static_assert(sizeof(MxRec) == 16, "one 16-byte vector per pair");

struct MxCounters { unsigned long long skipped, none; uint32_t err, pad; };

// One resolution.  A member's lifetime is the group it stands in, and mx_invalidate below is the only code that ends one: a new member
// goes into its group here and into the matching line there.
struct MxRes {
    // from create to destroy
    uint32_t r = 0;
    uint64_t nbins = 0;
    int B = 0;
    std::vector<uint32_t> off;
    DevBuf<uint32_t> d_off;
    // MX_NEW_CELLS: until the next add or run.  The cells, what is derived from them alone, and the times of the calls since
    uint64_t nnz = 0, text_bytes = 0;
    DevBuf<uint32_t> d_b1, d_b2, d_cnt;
    DevBuf<uint8_t> d_text;
    double ms = 0;
    MxLayout lay;                                   // built on demand by whoever needs it first
    ExpSetup exs;                                   // the grouping of the expected tables (mkt_matrix_expected)
    double bal_setup_ms = 0, bal_iter_ms = 0, exp_setup_ms = 0, exp_sums_ms = 0;
    // MX_NEW_WEIGHTS: ... or the next balance.  The weights and what may have been computed with them
    DevBuf<double> d_w;
    bool balanced = false;
    InsState ins;                                   // insulation scores and boundaries (mkt_matrix_insulation)
    SccState scc;                                   // replicate comparison (mkt_matrix_scc)
    // MX_NEW_TABLES: ... or the next expected.  The tables and what divides by them
    ExpTables ext;
    LoopsState lps;                                 // loop calling (mkt_matrix_loops)
    EigsState egs;                                  // compartment eigenvectors (mkt_matrix_eigs)
    PileState pile;                                 // pileup (mkt_matrix_pileup)
    SaddleState sad;                                // saddle tables (mkt_matrix_saddle)
};
// what has just become stale; each level ends what the one before it ends, and its own group
enum MxLevel { MX_NEW_TABLES, MX_NEW_WEIGHTS, MX_NEW_CELLS };
inline void mx_invalidate(MxRes& r, MxLevel level) {
    r.ext = ExpTables(); r.lps = LoopsState(); r.egs = EigsState(); r.pile = PileState(); r.sad = SaddleState();
    if (level == MX_NEW_TABLES) return;
    r.d_w.reset(); r.balanced = false; r.ins = InsState(); r.scc = SccState();
    if (level == MX_NEW_WEIGHTS) return;
    r.d_b1.reset(); r.d_b2.reset(); r.d_cnt.reset(); r.d_text.reset();
    r.nnz = 0; r.text_bytes = 0; r.lay = MxLayout(); r.exs = ExpSetup();
    r.ms = r.bal_setup_ms = r.bal_iter_ms = r.exp_setup_ms = r.exp_sums_ms = 0;
}

}  // namespace mkt

struct mkt_matrix {
    int device = 0;
    hipStream_t stream = nullptr;
    hipEvent_t ev0 = nullptr, ev1 = nullptr;
    std::vector<std::string> names;
    std::vector<uint32_t> lens;
    std::unordered_map<std::string, uint32_t> index;
    mkt::DevBuf<mkt::MxTab> d_tab;
    mkt::DevBuf<mkt::MxCounters> d_counters;
    mkt::DevBuf<mkt::MxRec> d_rec; uint64_t rec_cap = 0, n = 0;
    mkt::DevBuf<uint8_t> d_text; size_t text_cap = 0;
    std::string carry;                              // an incomplete last line of the text seen so far
    bool ran = false;
    uint64_t pairs = 0, skipped = 0;
    std::vector<mkt::MxRes> res;
    // per object, not per resolution: both live until the next add or run (mx_free_results in mkt_matrix.hip)
    mkt::VpState vp;                                // viewpoint profiles (mkt_matrix_viewpoint)
    mkt::HicState hic;                              // the .hic file (mkt_matrix_hic)
    std::string err;
};

namespace mkt {

extern thread_local std::string g_mx_create_err;   // what mkt_matrix_error(NULL) reads: one object, defined in mkt_matrix.hip
inline int mfail(mkt_matrix* m, int code, const char* fmt, ...) {
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    if (m) m->err = buf; else g_mx_create_err = buf;
    return code;
}
// a HIP error of section `sec` ("balance: ", ...); oom_own: out of memory has its own code there (the analyses and the run)
inline int mx_hip(mkt_matrix* m, const char* sec, hipError_t e, bool oom_own) {
    return mfail(m, oom_own && e == hipErrorOutOfMemory ? MKT_E_NOMEM : MKT_E_HIP, "%sHIP call failed: %s", sec, hipGetErrorString(e));
}
#define MX(m, sec, call) do { hipError_t e_ = (call); if (e_ != hipSuccess) return mx_hip((m), (sec), e_, true); } while (0)
#define MCHK(m, call) do { hipError_t e_ = (call); if (e_ != hipSuccess) return mx_hip((m), "", e_, false); } while (0)
// MX for an analysis that builds its results in place: a failure leaves `state` empty, not half made
#define MX_OR_RESET(m, sec, state, call) do { hipError_t e_ = (call); if (e_ != hipSuccess) { (state) = {}; return mx_hip((m), (sec), e_, true); } } while (0)

// what an entry point needs of a resolution before it may go on; each has its message
enum { MX_RAN = 1, MX_WEIGHTS = 2, MX_TABLES = 4, MX_LOOPS = 8, MX_EIGS = 16, MX_INS = 32, MX_PILE = 64, MX_SADDLE = 128, MX_SCC = 256 };
inline int mx_need(mkt_matrix* m, uint32_t res_index, const MxRes& r, int need, const char* what = nullptr) {
    if ((need & MX_RAN) && !m->ran) return mfail(m, MKT_E_STATE, "%s before run", what);
    if ((need & MX_WEIGHTS) && !(m->ran && r.balanced)) return mfail(m, MKT_E_STATE, "no weights for resolution index %u: balance first", res_index);
    if ((need & MX_TABLES) && !(m->ran && r.ext.built)) return mfail(m, MKT_E_STATE, "no expected tables for resolution index %u: expected first", res_index);
    if ((need & MX_LOOPS) && !(m->ran && r.lps.built)) return mfail(m, MKT_E_STATE, "no loops for resolution index %u: loops first", res_index);
    if ((need & MX_EIGS) && !(m->ran && r.egs.built)) return mfail(m, MKT_E_STATE, "no eigenvectors for resolution index %u: eigs first", res_index);
    if ((need & MX_INS) && !(m->ran && r.ins.built)) return mfail(m, MKT_E_STATE, "no insulation scores for resolution index %u: insulation first", res_index);
    if ((need & MX_PILE) && !(m->ran && r.pile.built)) return mfail(m, MKT_E_STATE, "no pileup for resolution index %u: pileup first", res_index);
    if ((need & MX_SADDLE) && !(m->ran && r.sad.built)) return mfail(m, MKT_E_STATE, "no saddle tables for resolution index %u: saddle first", res_index);
    if ((need & MX_SCC) && !(m->ran && r.scc.built)) return mfail(m, MKT_E_STATE, "no comparison for resolution index %u: scc first", res_index);
    return MKT_OK;
}
// the resolution of an entry point, or the error: the object, the index, then what it needs
inline int mx_res(mkt_matrix* m, uint32_t res_index, MxRes** r, int need = 0, const char* what = nullptr) {
    if (!m) return MKT_E_ARG;
    if (res_index >= m->res.size()) return mfail(m, MKT_E_ARG, "resolution index %u of %zu", res_index, m->res.size());
    *r = &m->res[res_index];
    return mx_need(m, res_index, **r, need, what);
}
#define MX_RES(...) do { const int rc_ = mx_res(__VA_ARGS__); if (rc_) return rc_; } while (0)
// the caller's options, or the defaults of the analysis
template <typename O>
O mx_opts(const O* opts, void (*defaults)(O*)) { O o; defaults(&o); return opts ? *opts : o; }
// the two refusals that several analyses word alike
inline int mx_cells32(mkt_matrix* m, const char* sec, uint64_t nnz) {
    if (nnz < (1ull << 32)) return MKT_OK;
    return mfail(m, MKT_E_CAPACITY, "%s: %llu cells: fewer than 2^32 are needed (cell indices are 32-bit)", sec, (unsigned long long)nnz);
}
inline int mx_kind(mkt_matrix* m, const char* sec, int kind) {
    if (kind == MKT_VALUE_BALANCED || kind == MKT_VALUE_OE || kind == MKT_VALUE_OE_SMOOTH) return MKT_OK;
    return mfail(m, MKT_E_ARG, "%s: kind %d (0 balanced, 1 oe, 2 oe_smooth)", sec, kind);
}
// the resident cells of a resolution, as the layout and the analyses take them
inline MxCells mx_cells(const MxRes& r) {
    MxCells c;
    c.b1 = r.d_b1; c.b2 = r.d_b2; c.cnt = r.d_cnt; c.off = r.d_off;
    c.nnz = r.nnz; c.nbins = r.nbins; c.nchr = (uint32_t)r.off.size(); c.B = r.B;
    return c;
}
// device time of work() between the object's two events; the stream is idle when it returns
template <typename F>
hipError_t mx_timed(mkt_matrix* m, double* ms_out, F&& work) {
    MKT_TRY(hipEventRecord(m->ev0, m->stream));
    MKT_TRY(work());
    MKT_TRY(hipEventRecord(m->ev1, m->stream));
    MKT_TRY(hipStreamSynchronize(m->stream));
    float ms = 0;
    MKT_TRY(hipEventElapsedTime(&ms, m->ev0, m->ev1));
    *ms_out = ms;
    return hipSuccess;
}
// one value of a *_timing getter: 0 until the analysis has results
inline void mx_ms(double* out, bool have, double ms) { if (out) *out = have ? ms : 0.0; }
template <typename T>
void mx_copy_rows(T* out, const std::vector<T>& v, uint64_t first, uint64_t n) { if (out && n) memcpy(out, v.data() + first, (size_t)n * sizeof(T)); }

}  // namespace mkt
