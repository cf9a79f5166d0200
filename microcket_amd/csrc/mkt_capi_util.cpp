// mkt_capi_util.cpp -- entry points of the C ABI beside the run itself: the synthetic generator and its data sets, uploads and
// copies for tests and tools, the diagnostic stamps.
#include "mkt_ctx.h"
#include <memory>

extern "C" {

int mkt_synth_device(mkt_ctx* c, uint64_t seed, int profile, int genome, int read_len, int lanes, uint64_t first_group,
                     uint64_t n_groups, int tail_group, const void** d_text, size_t* n_bytes) {
    if (!c || !d_text || !n_bytes) return MKT_E_ARG;
    HIPCHK(c, hipSetDevice(c->p.device));
    SynParams sp;
    sp.seed = seed; sp.profile = profile; sp.genome = genome; sp.read_len = read_len; sp.lanes = lanes;
    int rc = ensure(c, c->d_syn_sizes, n_groups + 2, n_groups + 2, false);
    if (rc) return rc;
    uint64_t* d_total = c->d_syn_sizes + n_groups;
    HIPCHK(c, launch_synth_sizes(sp, first_group, n_groups, c->d_syn_sizes, c->stream));
    HIPCHK(c, launch_exscan(c->d_syn_sizes, n_groups, d_total, c->stream));
    uint64_t total = 0;
    HIPCHK(c, hipMemcpyAsync(&total, d_total, sizeof total, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    size_t tail = tail_group ? synth_tail_bytes(sp) : 0;
    size_t need = (size_t)total + tail + 64;
    if ((rc = ensure(c, c->d_syn, need, need, false))) return rc;
    HIPCHK(c, launch_synth_write(sp, first_group, n_groups, c->d_syn_sizes, c->d_syn, c->stream));
    if (tail) HIPCHK(c, launch_synth_tail(sp, c->d_syn + total, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    *d_text = c->d_syn;
    *n_bytes = (size_t)total + tail;
    return MKT_OK;
}

struct mkt_dataset {
    mkt_ctx* ctx;
    DevBuf<char> arena;
    std::vector<uint64_t> off, len, groups;
    uint64_t total_bytes = 0, total_groups = 0;
};

int mkt_dataset_create(mkt_ctx* c, uint64_t seed, int profile, int genome, int read_len, int lanes, uint64_t first_group,
                       uint64_t n_groups, uint64_t gpb, int tail_group, mkt_dataset** out) {
    if (!c || !out || gpb == 0) return MKT_E_ARG;
    *out = nullptr;
    HIPCHK(c, hipSetDevice(c->p.device));
    SynParams sp;
    sp.seed = seed; sp.profile = profile; sp.genome = genome; sp.read_len = read_len; sp.lanes = lanes;
    const int rc = ensure(c, c->d_syn_sizes, gpb + 2, gpb + 2, false);
    if (rc) return rc;
    std::unique_ptr<mkt_dataset> ds(new mkt_dataset());      // (an early return below releases the arena with c's device current)
    ds->ctx = c;
    const uint64_t nb = (n_groups + gpb - 1) / gpb;
    const size_t tail = tail_group ? synth_tail_bytes(sp) : 0;
    uint64_t* d_total = c->d_syn_sizes + gpb;
    uint64_t cursor = 0;
    for (uint64_t b = 0; b < nb; ++b) {          // pass 1: block sizes
        const uint64_t g0 = b * gpb, g = (g0 + gpb <= n_groups) ? gpb : n_groups - g0;
        HIPCHK(c, launch_synth_sizes(sp, first_group + g0, g, c->d_syn_sizes, c->stream));
        HIPCHK(c, launch_exscan(c->d_syn_sizes, g, d_total, c->stream));
        uint64_t total = 0;
        HIPCHK(c, hipMemcpyAsync(&total, d_total, sizeof total, hipMemcpyDeviceToHost, c->stream));
        HIPCHK(c, hipStreamSynchronize(c->stream));
        if (b + 1 == nb) total += tail;
        if (total >= kMaxBlock) return fail(c, MKT_E_ARG, "block %llu would hold %llu bytes (>= 2 GiB - 64 KiB): lower groups_per_block", (unsigned long long)b, (unsigned long long)total);
        ds->off.push_back(cursor); ds->len.push_back(total); ds->groups.push_back(g + ((b + 1 == nb && tail_group) ? 1 : 0));
        cursor += (total + 15) & ~(uint64_t)15;
    }
    ds->total_bytes = 0;
    for (uint64_t l : ds->len) ds->total_bytes += l;
    ds->total_groups = n_groups + (tail_group ? 1 : 0);
    const hipError_t e = ds->arena.alloc(cursor + 64);
    if (e != hipSuccess) return fail(c, MKT_E_NOMEM, "hipMalloc of %llu bytes for the data set failed: %s", (unsigned long long)cursor, hipGetErrorString(e));
    for (uint64_t b = 0; b < nb; ++b) {          // pass 2: bytes
        const uint64_t g0 = b * gpb, g = (g0 + gpb <= n_groups) ? gpb : n_groups - g0;
        HIPCHK(c, launch_synth_sizes(sp, first_group + g0, g, c->d_syn_sizes, c->stream));
        HIPCHK(c, launch_exscan(c->d_syn_sizes, g, d_total, c->stream));
        HIPCHK(c, launch_synth_write(sp, first_group + g0, g, c->d_syn_sizes, ds->arena + ds->off[b], c->stream));
        if (b + 1 == nb && tail) HIPCHK(c, launch_synth_tail(sp, ds->arena + ds->off[b] + ds->len[b] - tail, c->stream));
        HIPCHK(c, hipStreamSynchronize(c->stream));
    }
    *out = ds.release();
    return MKT_OK;
}
int mkt_dataset_info(const mkt_dataset* ds, uint64_t* n_blocks, uint64_t* total_bytes, uint64_t* total_groups) {
    if (!ds) return MKT_E_ARG;
    if (n_blocks) *n_blocks = ds->off.size();
    if (total_bytes) *total_bytes = ds->total_bytes;
    if (total_groups) *total_groups = ds->total_groups;
    return MKT_OK;
}
int mkt_dataset_block(const mkt_dataset* ds, uint64_t i, const void** d_text, size_t* n_bytes, uint64_t* n_groups) {
    if (!ds || i >= ds->off.size()) return MKT_E_ARG;
    if (d_text) *d_text = ds->arena + ds->off[i];
    if (n_bytes) *n_bytes = (size_t)ds->len[i];
    if (n_groups) *n_groups = ds->groups[i];
    return MKT_OK;
}
void mkt_dataset_destroy(mkt_dataset* ds) {
    if (!ds) return;
    (void)hipSetDevice(ds->ctx->p.device);
    delete ds;
}

int mkt_group_count(mkt_ctx* c, uint64_t* groups) {
    if (!c || !groups) return MKT_E_ARG;
    int rc = mkt_sync(c);
    if (rc) return rc;
    *groups = c->acc.groups;
    return MKT_OK;
}

#if defined(MKT_STAMPS)
// diagnostic build only: per-phase shader-clock sums of k_tiles (see STAMP in mkt_kernels.hip)
int mkt_debug_stamps(mkt_ctx* c, unsigned long long* out16) {
    if (!c || !out16) return MKT_E_ARG;
    memset(out16, 0, 16 * sizeof(unsigned long long));
    if (!c->d_stamps) return MKT_OK;
    HIPCHK(c, hipStreamSynchronize(c->stream));
    HIPCHK(c, hipMemcpy(out16, c->d_stamps, 16 * sizeof(unsigned long long), hipMemcpyDeviceToHost));
    HIPCHK(c, hipMemset(c->d_stamps, 0, 16 * sizeof(unsigned long long)));
    return MKT_OK;
}
// diagnostic build only: the workgroup spans of k_fast since the last call (STAMP_SPAN in mkt_kernels.hip), 100 MHz ticks:
// sum of the spans, longest span, latest end, 2^62 - earliest first stamp
int mkt_debug_spans(mkt_ctx* c, unsigned long long* out4) {
    if (!c || !out4) return MKT_E_ARG;
    memset(out4, 0, 4 * sizeof(unsigned long long));
    if (!c->d_stamps) return MKT_OK;
    HIPCHK(c, hipStreamSynchronize(c->stream));
    HIPCHK(c, hipMemcpy(out4, c->d_stamps + 16, 4 * sizeof(unsigned long long), hipMemcpyDeviceToHost));
    HIPCHK(c, hipMemset(c->d_stamps + 16, 0, 4 * sizeof(unsigned long long)));
    return MKT_OK;
}
#endif

int mkt_device_text(mkt_ctx* c, const char* bytes, size_t n, const void** d_text) {
    if (!c || !d_text || (n && !bytes)) return MKT_E_ARG;
    HIPCHK(c, hipSetDevice(c->p.device));
    c->uploads.emplace_back();
    HIPCHK(c, c->uploads.back().alloc(n + 64));
    uint8_t* d = c->uploads.back();
    if (n) HIPCHK(c, hipMemcpy(d, bytes, n, hipMemcpyHostToDevice));
    *d_text = d;
    return MKT_OK;
}

int mkt_copy_to_host(mkt_ctx* c, const void* d_src, void* dst, size_t n) {
    if (!c || !d_src || !dst) return MKT_E_ARG;
    HIPCHK(c, hipSetDevice(c->p.device));
    HIPCHK(c, hipMemcpy(dst, d_src, n, hipMemcpyDeviceToHost));
    return MKT_OK;
}

}  // extern "C"
