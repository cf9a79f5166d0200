// mkt_capi.cpp -- the C ABI of include/mkt.h: contexts, block scheduling, host bookkeeping.
// Compiled with hipcc into libmkt_hip.so together with mkt_kernels.hip.  There is no CPU path:
// every entry point needs a HIP device and fails loudly without one.
#include "mkt_ctx.h"

extern "C" {

int mkt_abi_version(void) { return MKT_ABI_VERSION; }

const char* mkt_strerror(int code) {
    switch (code) {
    case MKT_OK: return "ok";
    case MKT_E_ARG: return "bad argument";
    case MKT_E_NO_DEVICE: return "no usable HIP device (this library has no CPU path)";
    case MKT_E_HIP: return "HIP runtime error";
    case MKT_E_NOMEM: return "out of memory";
    case MKT_E_CAPACITY: return "a QNAME group does not fit the block buffer";
    case MKT_E_KERNEL: return "kernel reported an internal error";
    case MKT_E_STATE: return "call order violated";
    case MKT_E_IO: return "temporary file error";
    case MKT_E_FORMAT: return "file refused";
    case MKT_E_RANGE: return "out of range";
    default: return "unknown error";
    }
}
const char* mkt_last_error(const mkt_ctx* ctx) { return ctx ? ctx->err.c_str() : g_create_error.c_str(); }

int mkt_device_count(void) {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) return 0;
    return n;
}

// the blocks' region buffers and the staged copies of the streaming path: an eighth and a page of slack
static int ensure_dev(mkt_ctx* c, GrowBuf<uint8_t>& b, size_t need) { return ensure(c, b, need, need + need / 8 + 4096, true); }

static hipError_t create_device_side(mkt_ctx* c) {
    MKT_TRY(hipSetDevice(c->p.device));
    MKT_TRY(c->stream.create(hipStreamNonBlocking));
    MKT_TRY(c->d_run.alloc(1));
    MKT_TRY(hipMemsetAsync(c->d_run, 0, sizeof(DevRun), c->stream));
    MKT_TRY(c->h_res.alloc(c->res_slots));
    return hipStreamSynchronize(c->stream);
}
int mkt_create(const mkt_params* p, mkt_ctx** out) {
    if (!p || !out) return fail(nullptr, MKT_E_ARG, "null argument");
    *out = nullptr;
    if (p->mode != MKT_MODE_FLASH && p->mode != MKT_MODE_UNC) return fail(nullptr, MKT_E_ARG, "mode must be MKT_MODE_FLASH or MKT_MODE_UNC");
    if (p->ref_threads < 2) return fail(nullptr, MKT_E_ARG, "ref_threads must be >= 2 (sam2pairs.cpp:36)");
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) return fail(nullptr, MKT_E_NO_DEVICE, "no HIP device: libmkt_hip has no CPU path");
    if (p->device < 0 || p->device >= ndev) return fail(nullptr, MKT_E_ARG, "device %d out of range (have %d)", p->device, ndev);
    mkt_ctx* c = new mkt_ctx();
    c->p = *p;
    c->P.mode = p->mode; c->P.ratio = p->min_mapped_ratio; c->P.min_mapq = (uint32_t)p->min_mapq; c->P.write_sam = p->write_sam ? 1 : 0;
    c->cfg = p->tiles == MKT_TILES_SMALL ? CFG_SMALL : CFG_FAST;
    c->dims = c->cfg == CFG_SMALL ? small_dims() : max_dims();
    c->dims_probed = p->tiles != MKT_TILES_AUTO || p->ordered;
    { const char* e = getenv("MKT_NO_LEAN"); c->no_lean = e && e[0] == '1'; }
    // rounds of the lean kernel's tiles held back for dealing by ticket: a number, or "all" = all but a workgroup's first tile
    if (const char* e = getenv("MKT_FAST_ROUNDS")) {
        char* end = nullptr;
        const unsigned long v = strtoul(e, &end, 10);
        if (!strcmp(e, "all")) c->fast_rounds = 0xFFFFFFFFu;
        else if (e[0] && end && !*end && v < 0xFFFFFFFFul) c->fast_rounds = (uint32_t)v;
        else { mkt_destroy(c); return fail(nullptr, MKT_E_ARG, "MKT_FAST_ROUNDS must be a number of rounds or \"all\""); }
    }
    size_t bc = p->block_bytes ? (size_t)p->block_bytes : ((size_t)64 << 20);
    if (bc < 4096) bc = 4096;
    if (bc >= kMaxBlock) bc = kMaxBlock - 4096;
    bc = (bc + 15) & ~(size_t)15;
    c->block_cap = bc;
    c->res_slots = 1024;
    const hipError_t e = create_device_side(c);
    if (e != hipSuccess) {
        mkt_destroy(c);
        fail(nullptr, MKT_E_HIP, "mkt_create failed: %s", hipGetErrorString(e));
        return e == hipErrorOutOfMemory ? MKT_E_NOMEM : MKT_E_HIP;
    }
    *out = c;
    return MKT_OK;
}

// only what has an order: the worker gone, the streams idle, then every member releases what it owns (the streams last)
void mkt_destroy(mkt_ctx* c) {
    if (!c) return;
    (void)hipSetDevice(c->p.device);
    if (c->worker_started) {
        { std::lock_guard<std::mutex> g(c->mu); c->stop = true; }
        c->cv.notify_all();
        c->worker.join();
    }
    (void)sync_all(c);
    delete c;
}

static int ensure_sc_list(mkt_ctx* c, size_t need);

// MKT_TILES_AUTO.  The bytes per tile follow the input's line length, looked at BEFORE the first launch (lines of the first MiB:
// counted by the host on the streaming path, by one small kernel on the resident path); lean_dims() turns it into a window
// of ~122 lines.  Should a block all the same leave more than one tile in eight to the generic kernel (the lines got shorter on
// the way), the following blocks use tiles of 0.6 x the bytes.
static void set_dims_from_avg(mkt_ctx* c, double bytes_per_line) {
    c->dims_probed = true;
    c->halo_widened = 0;
    if (c->cfg == CFG_SMALL || c->p.tiles != MKT_TILES_AUTO) return;
    c->dims = lean_dims(bytes_per_line);
    if (getenv("MKT_DEBUG_SYNC")) fprintf(stderr, "tile geometry: %.1f bytes per line -> tile %u, halos %u / %u\n", bytes_per_line, c->dims.tile, c->dims.hb, c->dims.hf);
}
static bool shrink_dims(mkt_ctx* c) {
    if (c->cfg == CFG_SMALL || c->dims.tile <= 2048u) return false;
    auto f = [](uint32_t x, uint32_t lo) { uint32_t y = ((uint32_t)(x * 0.6) + 15u) & ~15u; return y < lo ? lo : y; };
    c->dims.tile = f(c->dims.tile, 2048u); c->dims.hb = f(c->dims.hb, 256u); c->dims.hf = f(c->dims.hf, 512u);
    return true;
}
// halos half as wide again, the window as it was (the tile gives the bytes): for an input whose groups reach further than the
// default halos (many lines per read name), seen as tiles left to the generic kernel
static bool widen_halos(mkt_ctx* c) {
    if (c->cfg == CFG_SMALL || c->halo_widened >= 2) return false;
    const TileDims mx = max_dims();
    auto f = [](uint32_t x, uint32_t hi) { uint32_t y = ((uint32_t)(x * 1.5) + 15u) & ~15u; return y > hi ? hi : y; };
    const uint32_t hb = f(c->dims.hb, mx.hb), hf = f(c->dims.hf, mx.hf);
    const uint32_t delta = (hb - c->dims.hb) + (hf - c->dims.hf);
    if (delta == 0 || c->dims.tile < delta + 2048u) return false;
    c->dims.tile -= delta; c->dims.hb = hb; c->dims.hf = hf;
    ++c->halo_widened;
    if (getenv("MKT_DEBUG_SYNC")) fprintf(stderr, "tile geometry: halos widened -> tile %u, halos %u / %u\n", c->dims.tile, c->dims.hb, c->dims.hf);
    return true;
}
static bool adapt_geometry(mkt_ctx* c, const BlockResult& r) {
    if (c->p.tiles != MKT_TILES_AUTO || c->p.ordered) return false;
    if (r.tiles >= 1000 && (uint64_t)r.pad2 * 500 > r.tiles && widen_halos(c)) return true;      // more than 0.2 % of the tiles deferred for their halos
    if (r.tiles >= 8 && (uint64_t)(r.pad - r.pad2) * 8 > r.tiles) return shrink_dims(c);
    return false;
}
// bytes per line of device-resident text (its first MiB); the context's stream is idle afterwards.  0: could not tell
static double probe_device_lines(mkt_ctx* c, const uint8_t* d_text, size_t n) {
    const size_t look = n < ((size_t)1 << 20) ? n : ((size_t)1 << 20);
    if (!look) return 0;
    if (!c->h_probe && (c->d_probe.alloc(1) != hipSuccess || c->h_probe.alloc(1) != hipSuccess)) return 0;
    if (hipMemsetAsync(c->d_probe, 0, sizeof(unsigned long long), c->stream) != hipSuccess) return 0;
    if (launch_count_newlines(d_text, look, c->d_probe, c->stream) != hipSuccess) return 0;
    if (hipMemcpyAsync(c->h_probe, c->d_probe, sizeof(unsigned long long), hipMemcpyDeviceToHost, c->stream) != hipSuccess) return 0;
    if (hipStreamSynchronize(c->stream) != hipSuccess) return 0;
    return *c->h_probe ? (double)look / (double)*c->h_probe : (double)look;
}
// a block came back with its line table overflown (E_LINE_TABLE: its lines are shorter than the geometry was chosen for): tiles
// for ITS line length if that makes them smaller, else 0.6 x the bytes, in the end the 256-byte tiles
static void smaller_geometry(mkt_ctx* c, const uint8_t* d_text, size_t n) {
    if (c->cfg != CFG_SMALL && d_text) {
        const double avg = probe_device_lines(c, d_text, n);
        const TileDims d = avg > 0 ? lean_dims(avg) : c->dims;
        if (d.tile < c->dims.tile) { c->dims = d; return; }
    }
    if (!shrink_dims(c)) { c->cfg = CFG_SMALL; c->dims = small_dims(); }
}

// ---------------------------------------------------------------------------------------------
// enqueue one block: memset workspace, tile kernel (timed), finish kernel, result D2H into slot.
// so (streaming path): the block's outputs are also gathered into the contiguous buffers of an output slot, the timing
// events are the input slot's own, and `done` is recorded behind everything.
struct StreamOut { uint8_t* gp; size_t gp_cap; uint8_t* gs; size_t gs_cap; hipEvent_t k0, k1, done; };
static int enqueue_block(mkt_ctx* c, const uint8_t* d_text, size_t n, int cfg, const TileDims& dims, size_t slot, const StreamOut* so = nullptr) {
    if (((uintptr_t)d_text & 15u) != 0) return fail(c, MKT_E_ARG, "block text must be 16-byte aligned");
    if (n >= kMaxBlock) return fail(c, MKT_E_ARG, "block of %zu bytes: must be < 2 GiB - 64 KiB", n);
    const uint32_t ntiles = num_tiles((uint32_t)n, dims.tile);
    BlockWs ws{nullptr, ntiles};
    const size_t ws_bytes = ws.bytes();
    int rc = ensure(c, c->d_ws, ws_bytes, ws_bytes + ws_bytes / 4, true);
    if (rc) return rc;
    ws.base = c->d_ws;
    if ((ntiles + finish_chunk_tiles() - 1) / finish_chunk_tiles() > BlockWs::kScanWords) return fail(c, MKT_E_ARG, "block has too many tiles for the finish scan");
    // output capacities: .sam is at most the block (+1 for a missing final newline); .pairs is
    // checked in-kernel and grown on demand (the result carries the exact size)
    if ((rc = ensure_dev(c, c->d_pairs, n / 3 + 65536))) return rc;
    if (c->P.write_sam && (rc = ensure_dev(c, c->d_sam, n + n / 4 + 65536))) return rc;
    if (!c->d_sc && (rc = ensure_sc_list(c, 1))) return rc;
    KArgs a;
    memset(&a, 0, sizeof a);
    a.text = d_text; a.n = (uint32_t)n; a.ntiles = ntiles; a.dims = dims; a.P = c->P;
    a.descA = ws.descA(); a.descB = ws.descB(); a.descC = ws.descC();
    a.tile_last = ws.tile_last(); a.tile_groups = ws.tile_groups(); a.defer_list = ws.defer_list();
    a.cur = ws.cur();
    a.ticket = ws.ticket(); a.defer_count = ws.defer_count(); a.fast_ticket = ws.fast_ticket();
    a.last_tile = ws.last_tile(); a.scan_ticket = ws.scan_ticket(); a.scan_desc = ws.scan_desc();
    a.res = ws.res();
    a.ordered = c->p.ordered ? 1 : 0;
    a.run = c->d_run;
    // any-order mode: outputs in kMaxRegions equal slices (one cursor line each); ordered mode: one region
    a.nregions = c->p.ordered ? 1 : kMaxRegions;
    const size_t sc_need = (size_t)a.nregions * ((n / 256 / (size_t)a.nregions) * 2 + 1024);
    if ((rc = ensure(c, c->d_sc_tmp, sc_need, sc_need, true))) return rc;
    a.pairs_rcap = (c->d_pairs.cap() / a.nregions) & ~(uint64_t)15;
    a.sam_rcap = c->P.write_sam ? ((c->d_sam.cap() / a.nregions) & ~(uint64_t)15) : 0;
    a.sc_rcap = c->d_sc_tmp.cap() / a.nregions;
    a.out.pairs = c->d_pairs; a.out.pairs_cap = c->d_pairs.cap();
    a.out.sam = c->d_sam; a.out.sam_cap = c->P.write_sam ? c->d_sam.cap() : 0;
    a.out.sc = c->d_sc_tmp; a.out.sc_cap = c->d_sc_tmp.cap();
    a.sc_list = c->d_sc; a.sc_list_cap = c->d_sc.cap();
    if (c->p.extensions & MKT_EXT_KEYS) {
        if (!c->d_chr) { HIPCHK(c, c->d_chr.alloc(1)); HIPCHK(c, hipMemsetAsync(c->d_chr, 0, sizeof(ChrTab), c->stream)); }
        // at most one reported pair per two 32-byte lines; twice that per region for imbalance
        const size_t per = (n / 64 / (size_t)a.nregions) * 2 + 4096, need = per * a.nregions;
        if ((rc = ensure(c, c->d_keys_raw, need, need, true))) return rc;
        // the run's list grows by doubling (the stream is idle whenever it has to: growth syncs)
        // room for the records of the blocks in flight: one pair per 64 input bytes until a sync has shown this input's
        // density, afterwards twice the highest density seen (k_finish checks the real count: too small is an error)
        const double per_byte = c->key_density > 0 ? (c->key_density * 2 < 1.0 / 64 ? c->key_density * 2 : 1.0 / 64) : 1.0 / 64;
        const size_t want = (size_t)c->acc.emitted + (size_t)((double)(c->bytes_unsynced + n) * per_byte) + 65536;
        if (!c->d_key_list.fits(want)) {
            size_t ncap = c->d_key_list.cap() ? c->d_key_list.cap() * 2 : ((size_t)1 << 22);
            while (ncap < want) ncap *= 2;
            HIPCHK(c, hipStreamSynchronize(c->stream));
            HIPCHK(c, c->d_key_list.regrow_keep(ncap, c->d_key_list.cap()));
        }
        a.keys_rcap = c->d_keys_raw.cap() / a.nregions;
        a.out.keys = c->d_keys_raw; a.out.keys_cap = c->d_keys_raw.cap(); a.out.chr = c->d_chr;
        a.out.key_lanes = (c->p.extensions & MKT_EXT_LANES) ? 1u : 0u;
        a.key_list = c->d_key_list; a.key_list_cap = c->d_key_list.cap();
    }
#if defined(MKT_STAMPS)
    if (!c->d_stamps) { HIPCHK(c, c->d_stamps.alloc(kStampWords)); HIPCHK(c, hipMemset(c->d_stamps, 0, kStampWords * sizeof(unsigned long long))); }
    a.stamps = getenv("MKT_NO_STAMPS") ? nullptr : c->d_stamps;
    { const char* e = getenv("MKT_DEBUG_STOP"); a.debug_stop = e ? atoi(e) : 0; }
#endif
    HIPCHK(c, hipMemsetAsync(c->d_ws, 0, ws_bytes, c->stream));
    hipEvent_t e0, e1;
    if (so) { e0 = so->k0; e1 = so->k1; }
    else {
        c->ev.emplace_back();                             // (a pair that could not be created counts nothing: fold_timing)
        c->ev.back().bytes = n;
        HIPCHK(c, c->ev.back().ev.create());
        e0 = c->ev.back().ev[0]; e1 = c->ev.back().ev[1];
    }
    const uint32_t max_wgs = fast_max_workgroups(cfg);       // every workgroup resident
    int grid = (int)(ntiles < max_wgs ? ntiles : max_wgs);
    // lean kernel: rounds 0 .. K-1 of its tiles are dealt statically (tile = workgroup + k * grid), K = max(1, ntiles / grid - R); the
    // tiles behind them, R whole rounds and the partial one, by ticket.  R = 0 (or a block of one round): every tile static.
    a.fast_dyn0 = kFastAllStatic;
    if (c->fast_rounds && ntiles > (uint32_t)grid) {
        const uint32_t rounds = ntiles / (uint32_t)grid, K = rounds > c->fast_rounds ? rounds - c->fast_rounds : 1u;
        a.fast_dyn0 = K * (uint32_t)grid;
    }
#if defined(MKT_STAMPS)
    if (a.debug_stop) a.fast_dyn0 = kFastAllStatic;                  // (the timing ladder leaves tiles early, before the next ticket is drawn)
#endif
    const bool lean = !c->p.ordered && cfg != CFG_SMALL && !c->no_lean;
    HIPCHK(c, hipEventRecord(e0, c->stream));
    if (lean) {
        // lean kernel over all tiles, then the generic kernel over the tiles it deferred
        HIPCHK(c, launch_fast(a, cfg, grid, c->stream));
        HIPCHK(c, hipEventRecord(e1, c->stream));
        KArgs b = a;
        b.use_list = 1; b.ticket = ws.defer_ticket();
        HIPCHK(c, launch_tiles(b, cfg, ntiles < 96u ? (int)ntiles : 96, c->stream));
    } else {
        HIPCHK(c, launch_tiles(a, cfg, grid, c->stream));
        HIPCHK(c, hipEventRecord(e1, c->stream));
    }
    HIPCHK(c, launch_finish(a, c->stream));
    if (so) {
        const uint64_t prc = a.nregions > 1 ? a.pairs_rcap : 0, src_ = a.nregions > 1 ? a.sam_rcap : 0;
        HIPCHK(c, launch_gather(a.res, c->d_pairs, prc, so->gp, so->gp_cap, 0, n / 8, c->stream));
        if (c->P.write_sam) HIPCHK(c, launch_gather(a.res, c->d_sam, src_, so->gs, so->gs_cap, 1, n, c->stream));
    }
    HIPCHK(c, hipMemcpyAsync(&c->h_res[slot], a.res, sizeof(BlockResult), hipMemcpyDeviceToHost, c->stream));
    if (so) HIPCHK(c, hipEventRecord(so->done, c->stream));
    return MKT_OK;
}

static void fold_timing(mkt_ctx* c) {       // stream must be idle
    for (const mkt_ctx::Timed& t : c->ev) {
        float ms = 0;
        if (hipEventElapsedTime(&ms, t.ev[0], t.ev[1]) == hipSuccess) { c->folded_ms += ms; ++c->folded_launches; c->folded_bytes += t.bytes; }
    }
    c->ev.clear();
}

// The run's resolved self-circle indices stay on the device until the end of the input (k_sc_logged).
// Stream idle: make room for `need` entries, keeping the c->acc.sc entries already there.
static int ensure_sc_list(mkt_ctx* c, size_t need) {
    if (c->d_sc.fits(need)) return MKT_OK;
    size_t ncap = c->d_sc.cap() ? c->d_sc.cap() : ((size_t)1 << 20);       // 1 Mi entries (8 MiB) at least; the resident path asks for its first 2 GB block's worth at once
    while (ncap < need) ncap *= 2;
    HIPCHK(c, c->d_sc.regrow_keep(ncap, c->d_sc.get() ? (size_t)c->acc.sc : 0));
    return MKT_OK;
}
// after a sync: what this input's self-circle density looks like (entries per input byte, highest seen)
static void note_sc_density(mkt_ctx* c) {
    if (c->bytes_unsynced) {
        const double d = (double)c->sc_unfolded / (double)c->bytes_unsynced;
        if (d > c->sc_density) c->sc_density = d;
        if (c->sc_density == 0) c->sc_density = 1e-12;   // seen, none so far
        const double k = (double)c->emitted_unfolded / (double)c->bytes_unsynced;
        if (k > c->key_density) c->key_density = k;
        if (c->key_density == 0) c->key_density = 1e-12;
    }
    c->sc_unfolded = 0; c->bytes_unsynced = 0; c->emitted_unfolded = 0;
}
// entries the next `bytes` of input may add at most, as far as the host can tell: one group per 64 bytes until a sync
// has shown this input's density, afterwards 4 x the highest density seen and at least one per 65536 bytes.  k_finish
// checks the real count against the capacity: a wrong guess is an error (E_SC_CAP), never a silent loss.
static size_t sc_estimate(const mkt_ctx* c, size_t bytes) {
    const double per_byte = c->sc_density > 0 ? (c->sc_density * 4 > 1.0 / 65536 ? c->sc_density * 4 : 1.0 / 65536) : 1.0 / 64;
    return (size_t)((double)bytes * per_byte) + 4096;
}

static int check_result(mkt_ctx* c, const BlockResult& r) {
    if (r.err == 0) return MKT_OK;
    return fail(c, MKT_E_KERNEL, "kernel error bits 0x%x%s%s%s%s%s%s", r.err,
                (r.err & E_LINE_TABLE) ? " [line table overflow: use MKT_TILES_SMALL]" : "",
                (r.err & E_LOOKBACK) ? " [look-back timeout]" : "",
                (r.err & E_PAIRS_CAP) ? " [.pairs buffer]" : "", (r.err & E_SAM_CAP) ? " [.sam buffer]" : "",
                (r.err & E_SC_CAP) ? " [self-circle buffer]" : "", (r.err & E_FIELD_RANGE) ? " [field > 65535 bytes]" : "");
}

// ---------------------------------------------------------------------------------------------
// Streaming path.  Caller thread: fills input slot `cur`, cuts it on a group boundary, queues H2D + kernels + gather for
// the prefix and moves on to the next slot with the carry.  Worker thread: per job, in order -- wait for the result, fold
// it into the run, copy the gathered outputs into a pinned staging slot, hold back the block's last group (quirk Q1),
// publish the rest.  Everything shared is guarded by c->mu; blocking waits on the GPU happen outside it.

static int stream_start(mkt_ctx* c) {
    if (!c->s_in) HIPCHK(c, c->s_in.create(hipStreamNonBlocking));
    if (!c->s_out) HIPCHK(c, c->s_out.create(hipStreamNonBlocking));
    return MKT_OK;
}
static int stream_alloc_in(mkt_ctx* c, int i) {
    mkt_ctx::InSlot& s = c->in[i];
    if (!s.h) HIPCHK(c, s.h.alloc(c->block_cap + 64));
    return MKT_OK;
}
static int stream_alloc_dev(mkt_ctx* c, int i) {
    mkt_ctx::InSlot& s = c->in[i];
    if (!s.d) HIPCHK(c, s.d.alloc(c->block_cap + 64));
    if (!s.ev[mkt_ctx::EV_DONE]) {
        HIPCHK(c, s.ev.create(mkt_ctx::EV_H2D, hipEventDisableTiming));
        HIPCHK(c, s.ev.create(mkt_ctx::EV_K0, 0));
        HIPCHK(c, s.ev.create(mkt_ctx::EV_K1, 0));
        HIPCHK(c, s.ev.create(mkt_ctx::EV_DONE, hipEventDisableTiming));
    }
    return MKT_OK;
}
static void worker_main(mkt_ctx* c);

// queue the GPU work of one job (c->mu held; the job's input is in d_in already or on its way on s_in)
static int stream_launch(mkt_ctx* c, const mkt_ctx::Job& j) {
    mkt_ctx::InSlot& is = c->in[j.in_slot];
    mkt_ctx::OutSlot& os = c->outs[j.out_slot];
    int rc;
    // the region buffers are sized here once for a whole block (never regrown in flight except by a replay, which is idle)
    if ((rc = ensure_dev(c, c->d_pairs, c->block_cap / 3 + 65536))) return rc;
    if (c->P.write_sam && (rc = ensure_dev(c, c->d_sam, c->block_cap + c->block_cap / 4 + 65536))) return rc;
    if ((rc = ensure_dev(c, os.d_pairs, c->d_pairs.cap()))) return rc;
    if (c->P.write_sam && (rc = ensure_dev(c, os.d_sam, c->d_sam.cap()))) return rc;
    StreamOut so;
    so.gp = os.d_pairs; so.gp_cap = os.d_pairs.cap(); so.gs = os.d_sam; so.gs_cap = os.d_sam.cap();
    so.k0 = is.ev[mkt_ctx::EV_K0]; so.k1 = is.ev[mkt_ctx::EV_K1]; so.done = is.ev[mkt_ctx::EV_DONE];
    return enqueue_block(c, is.d, j.n, j.cfg, j.dims, c->res_slots - mkt_ctx::kIn + (size_t)j.in_slot, &so);
}

// c->mu held by lk.  Hands input slot `slot` (n bytes) to the GPU.
static int stream_enqueue(mkt_ctx* c, std::unique_lock<std::mutex>& lk, int slot, size_t n) {
    int rc;
    if ((rc = stream_start(c))) return rc;
    const int oslot = (int)(c->seq % mkt_ctx::kOut);
    // the output slot's device buffers are free once the job two back has been copied out
    c->cv.wait(lk, [&] { return c->async_rc != MKT_OK || !c->outs[oslot].dev_busy; });
    if (c->async_rc) return c->async_rc;
    // room in the run's self-circle list for every block in flight at one group per 64 input bytes; growing it needs the
    // pipeline idle (only the entries of folded blocks are carried over)
    const size_t per_block = c->block_cap / 64 + 4096;
    if (!c->d_sc || (size_t)c->acc.sc + (c->jobs.size() + 1) * per_block > c->d_sc.cap()) {
        c->cv.wait(lk, [&] { return c->async_rc != MKT_OK || c->jobs.empty(); });
        if (c->async_rc) return c->async_rc;
        if ((rc = ensure_sc_list(c, 2 * (size_t)c->acc.sc + (size_t)(mkt_ctx::kOut + 1) * per_block))) return rc;
    }
    if ((rc = stream_alloc_dev(c, slot))) return rc;
    mkt_ctx::InSlot& is = c->in[slot];
    HIPCHK(c, hipMemcpyAsync(is.d, is.h, n, hipMemcpyHostToDevice, c->s_in));
    HIPCHK(c, hipEventRecord(is.ev[mkt_ctx::EV_H2D], c->s_in));
    HIPCHK(c, hipStreamWaitEvent(c->stream, is.ev[mkt_ctx::EV_H2D], 0));
    if (!c->dims_probed) {                                 // the input's line length, from the first MiB (in pinned host memory)
        const size_t look = n < ((size_t)1 << 20) ? n : ((size_t)1 << 20);
        size_t lines = 0;
        for (const uint8_t* q = is.h.get(), *e = q + look; q < e && (q = (const uint8_t*)memchr(q, '\n', (size_t)(e - q))); ++q) ++lines;
        set_dims_from_avg(c, lines ? (double)look / (double)lines : (double)look);
    }
    mkt_ctx::Job j;
    j.in_slot = slot; j.out_slot = oslot; j.n = n; j.cfg = c->cfg; j.dims = c->dims; j.attempts = 0;
    c->bytes_unsynced = 0;
    for (const mkt_ctx::Job& q : c->jobs) c->bytes_unsynced += q.n;     // extension: key-list reservation covers the blocks in flight
    if ((rc = stream_launch(c, j))) return rc;
    is.busy = true; c->outs[oslot].dev_busy = true;
    c->jobs.push_back(j);
    ++c->seq;
    if (!c->worker_started) { c->worker_started = true; c->worker = std::thread(worker_main, c); }
    c->cv.notify_all();
    return MKT_OK;
}

// the run totals on the device go back to what the folded blocks left (before blocks are run again; the stream is idle)
static int rewind_run(mkt_ctx* c) {
    DevRun dr;
    dr.groups = c->acc.groups; dr.sc = c->acc.sc; dr.emitted = c->acc.emitted;
    HIPCHK(c, hipMemcpy(c->d_run, &dr, sizeof dr, hipMemcpyHostToDevice));
    return MKT_OK;
}
// A job came back with error bits (c->mu held, worker thread): fix the cause the way a synchronous run would -- next
// smaller tile geometry, bigger output buffers -- and run it again, followed by every job queued behind it (they ran on
// top of run totals that the failed block never advanced).  Inputs are still in their device slots.
static int stream_replay(mkt_ctx* c, const BlockResult& r) {
    int rc;
    if ((rc = sync_all(c))) return rc;
    mkt_ctx::Job& j0 = c->jobs.front();
    if (++j0.attempts > 4) return check_result(c, r);
    bool fixed = false;
    if ((r.err & (E_LINE_TABLE | E_OVF_SLOTS)) && j0.cfg != CFG_SMALL && c->p.tiles == MKT_TILES_AUTO) {
        const int keep_cfg = c->cfg; const TileDims keep = c->dims;
        c->cfg = j0.cfg; c->dims = j0.dims;
        smaller_geometry(c, c->in[j0.in_slot].d, j0.n);
        for (mkt_ctx::Job& q : c->jobs) { q.cfg = c->cfg; q.dims = c->dims; }
        if (c->cfg == CFG_SMALL) { c->cfg = keep_cfg; c->dims = keep; }      // (the 256-byte tiles are a last resort per block: the stream keeps its lean geometry)
        ++c->replays.geometry;
        fixed = true;
    } else {
        const uint32_t nr = r.nregions ? r.nregions : 1;
        if (r.err & E_PAIRS_CAP) {
            uint64_t mx = 0; for (uint32_t q = 0; q < nr; ++q) if (r.rpair[q] > mx) mx = r.rpair[q];
            if ((rc = ensure_dev(c, c->d_pairs, (size_t)(mx * nr) + mx / 4 * nr + 65536))) return rc;
            ++c->replays.pairs_cap;
            fixed = true;
        }
        if (r.err & E_SAM_CAP) {
            uint64_t mx = 0; for (uint32_t q = 0; q < nr; ++q) if (r.rsam[q] > mx) mx = r.rsam[q];
            if ((rc = ensure_dev(c, c->d_sam, (size_t)(mx * nr) + mx / 4 * nr + 65536))) return rc;
            ++c->replays.sam_cap;
            fixed = true;
        }
        if (r.err & E_SC_CAP) {            // per-block raw entries: grow the slices, and the run's list with them
            const size_t need = (size_t)r.sc * 4 + 65536;
            HIPCHK(c, c->d_sc_tmp.regrow(need * kMaxRegions));         // (idle already; whatever its size was)
            if ((rc = ensure_sc_list(c, (size_t)c->acc.sc + (c->jobs.size() + 1) * need))) return rc;
            c->key_density = 0;            // extension: the key list may be what overflowed: back to the worst-case reservation
            ++c->replays.sc_cap;
            fixed = true;
        }
    }
    if (!fixed) return check_result(c, r);
    if ((rc = rewind_run(c))) return rc;
    c->bytes_unsynced = 0;
    for (const mkt_ctx::Job& q : c->jobs) {
        if ((rc = stream_launch(c, q))) return rc;
        c->bytes_unsynced += q.n;
        ++c->replays.jobs_rerun;
    }
    return MKT_OK;
}

static void worker_fail(mkt_ctx* c, int rc) {       // c->mu held
    if (c->async_rc == MKT_OK) c->async_rc = rc ? rc : MKT_E_HIP;
    c->cv.notify_all();
}

static void worker_main(mkt_ctx* c) {
    (void)hipSetDevice(c->p.device);
    std::unique_lock<std::mutex> lk(c->mu);
    for (;;) {
        c->cv.wait(lk, [&] { return c->stop || (!c->jobs.empty() && c->async_rc == MKT_OK); });
        if (c->stop) return;
        const mkt_ctx::Job j = c->jobs.front();
        hipEvent_t done = c->in[j.in_slot].ev[mkt_ctx::EV_DONE];
        lk.unlock();
        hipError_t he = hipEventSynchronize(done);
        lk.lock();
        if (c->stop) return;
        if (he != hipSuccess) { fail(c, MKT_E_HIP, "hipEventSynchronize failed: %s", hipGetErrorString(he)); worker_fail(c, MKT_E_HIP); continue; }
        const BlockResult r = c->h_res[c->res_slots - mkt_ctx::kIn + (size_t)j.in_slot];
        if (r.err) {
            const int rc = stream_replay(c, r);
            if (rc) worker_fail(c, rc);
            continue;                                  // wait for the re-run of the same job
        }
        // ---- fold the block into the run
        c->acc.add_block(r); c->tiles_total += r.tiles; c->tiles_deferred += r.pad; adapt_geometry(c, r);
        ++c->blocks;
        c->sc_unfolded += r.sc; c->emitted_unfolded += r.emitted; c->bytes_unsynced = j.n;
        note_sc_density(c);
        {
            float ms = 0;
            mkt_ctx::InSlot& is = c->in[j.in_slot];
            if (hipEventElapsedTime(&ms, is.ev[mkt_ctx::EV_K0], is.ev[mkt_ctx::EV_K1]) == hipSuccess) { c->folded_ms += ms; ++c->folded_launches; c->folded_bytes += j.n; }
        }
        const size_t pb = (size_t)r.pair_bytes, sb = c->P.write_sam ? (size_t)r.sam_bytes : 0;
        mkt_ctx::OutSlot& os = c->outs[j.out_slot];
        // ---- copy the gathered outputs out (the staging slot must be back from the consumer)
        while (os.host_busy && !c->stop) {
            if (!c->consumer_async) {
                // single-threaded caller (submit ... drain later): nobody will release the slot while the caller is inside
                // mkt_submit, so its published chunk moves to the heap instead
                for (mkt_ctx::Chunk& q : c->ready)
                    if (q.out_slot == j.out_slot) {
                        q.own_pairs.assign(q.pairs, q.pairs + q.pairs_len); q.own_sam.assign(q.sam, q.sam + q.sam_len);
                        q.pairs = q.own_pairs.data(); q.sam = q.own_sam.data(); q.out_slot = -1;
                    }
                if (!(c->handed_valid && c->handed.out_slot == j.out_slot)) { os.host_busy = false; break; }
            }
            c->cv.wait(lk);
        }
        if (c->stop) return;
        const size_t H = mkt_ctx::kHead;
        const size_t sam_at = ((H + pb + 4095) & ~(size_t)4095) + H, need = sam_at + sb + 64;
        bool bad = false;
        if (pb + sb) {
            const size_t want = need + need / 4;
            if (!os.h.fits(need) && os.h.regrow(want) != hipSuccess) { fail(c, MKT_E_NOMEM, "pinned staging of %zu bytes", want); worker_fail(c, MKT_E_NOMEM); bad = true; }
            if (!bad) {
                lk.unlock();
                hipError_t e1 = pb ? hipMemcpyAsync(os.h + H, os.d_pairs, pb, hipMemcpyDeviceToHost, c->s_out) : hipSuccess;
                hipError_t e2 = sb ? hipMemcpyAsync(os.h + sam_at, os.d_sam, sb, hipMemcpyDeviceToHost, c->s_out) : hipSuccess;
                hipError_t e3 = hipStreamSynchronize(c->s_out);
                lk.lock();
                if (e1 != hipSuccess || e2 != hipSuccess || e3 != hipSuccess) { fail(c, MKT_E_HIP, "output copy failed"); worker_fail(c, MKT_E_HIP); bad = true; }
            }
        }
        if (c->stop) return;
        if (bad) continue;
        // ---- quirk Q1: the newest group stays back until a later group supersedes it
        mkt_ctx::Chunk ch;
        ch.out_slot = j.out_slot;
        const char* hp = (const char*)os.h.get() + H;
        const char* hs = (const char*)os.h.get() + sam_at;
        if (r.last.valid) {
            const size_t tp = r.last.pair_bytes, ts = c->P.write_sam ? r.last.sam_bytes : 0;      // gathered layout: [ the rest | last group ]
            const size_t bp = pb - tp, bs = sb - ts;
            ch.pairs = hp; ch.pairs_len = bp; ch.sam = hs; ch.sam_len = bs;
            if (!c->tail_pairs.empty() || !c->tail_sam.empty()) {
                if (pb + sb && c->tail_pairs.size() <= H && c->tail_sam.size() <= H) {             // in front of this block's bytes
                    if (!c->tail_pairs.empty()) { memcpy(os.h + H - c->tail_pairs.size(), c->tail_pairs.data(), c->tail_pairs.size()); ch.pairs = hp - c->tail_pairs.size(); ch.pairs_len += c->tail_pairs.size(); }
                    if (!c->tail_sam.empty()) { memcpy(os.h + sam_at - c->tail_sam.size(), c->tail_sam.data(), c->tail_sam.size()); ch.sam = hs - c->tail_sam.size(); ch.sam_len += c->tail_sam.size(); }
                } else {                                                                           // as a chunk of its own
                    mkt_ctx::Chunk t;
                    t.own_pairs.swap(c->tail_pairs); t.own_sam.swap(c->tail_sam);
                    c->ready.push_back(std::move(t));
                }
            }
            if (tp) c->tail_pairs.assign(hp + bp, hp + bp + tp); else c->tail_pairs.clear();
            if (ts) c->tail_sam.assign(hs + bs, hs + bs + ts); else c->tail_sam.clear();
        } else {
            ch.pairs = hp; ch.pairs_len = pb; ch.sam = hs; ch.sam_len = sb;                        // a block without any group reports nothing
        }
        if (ch.pairs_len + ch.sam_len) { os.host_busy = true; c->ready.push_back(std::move(ch)); }
        os.dev_busy = false;
        c->in[j.in_slot].busy = false;
        c->jobs.pop_front();
        c->cv.notify_all();
    }
}

// c->mu held by lk: every queued job folded (or an error)
static int stream_wait_idle(mkt_ctx* c, std::unique_lock<std::mutex>& lk) {
    c->cv.wait(lk, [&] { return c->async_rc != MKT_OK || c->jobs.empty(); });
    return c->async_rc;
}

// the input slot is full (or the input ended): queue its group-aligned prefix, carry the rest into the next slot
static int stream_flush(mkt_ctx* c, bool everything) {
    std::unique_lock<std::mutex> lk(c->mu);
    if (c->async_rc) return c->async_rc;
    mkt_ctx::InSlot& is = c->in[c->cur];
    if (everything) {
        if (c->h_len) { int rc = stream_enqueue(c, lk, c->cur, c->h_len); if (rc) return rc; }
        c->cur = (c->cur + 1) % mkt_ctx::kIn;
        c->h_len = 0;
        return MKT_OK;
    }
    size_t end = 0;
    const size_t cut = group_aligned_prefix((const char*)is.h.get(), c->h_len, c->P.min_mapq, &end);
    if (cut == 0) {
        // one group (or none closed) in the whole slot: lines that the filter drops influence nothing, squeeze them out
        const size_t nl = compact_carry((char*)is.h.get(), c->h_len, c->P.min_mapq);
        if (nl + 4096 > c->h_len || nl + 4096 > c->block_cap)
            return fail(c, MKT_E_CAPACITY, "no QNAME-group boundary inside a %zu-byte block: raise block_bytes", c->block_cap);
        c->h_len = nl;
        return MKT_OK;
    }
    const int next = (c->cur + 1) % mkt_ctx::kIn;
    c->cv.wait(lk, [&] { return c->async_rc != MKT_OK || !c->in[next].busy; });
    if (c->async_rc) return c->async_rc;
    int rc = stream_alloc_in(c, next);
    if (rc) return rc;
    size_t carry = c->h_len - cut;
    memcpy(c->in[next].h, is.h + cut, carry);
    if (carry > c->block_cap / 2) carry = compact_carry((char*)c->in[next].h.get(), carry, c->P.min_mapq);
    if ((rc = stream_enqueue(c, lk, c->cur, cut))) return rc;
    c->cur = next;
    c->h_len = carry;
    return MKT_OK;
}

static int stream_check_open(mkt_ctx* c) {
    if (c->input_done || c->finished) return fail(c, MKT_E_STATE, "input after the end of input");
    { std::lock_guard<std::mutex> g(c->mu); if (c->async_rc) return c->async_rc; }
    HIPCHK(c, hipSetDevice(c->p.device));
    return stream_alloc_in(c, c->cur);
}

int mkt_submit(mkt_ctx* c, const char* bytes, size_t n, int last) {
    if (!c) return MKT_E_ARG;
    if (n && !bytes) return fail(c, MKT_E_ARG, "null bytes");
    int rc = stream_check_open(c);
    if (rc) return rc;
    size_t pos = 0;
    c->bytes_in += n;
    for (;;) {
        size_t space = c->block_cap - c->h_len;
        size_t take = n - pos < space ? n - pos : space;
        if (take) { memcpy(c->in[c->cur].h + c->h_len, bytes + pos, take); c->h_len += take; pos += take; }
        const bool all_in = pos == n;
        if (c->h_len == c->block_cap && !(all_in && last)) {
            if ((rc = stream_flush(c, false))) return rc;
            if ((rc = stream_alloc_in(c, c->cur))) return rc;
            continue;
        }
        if (all_in) break;
    }
    if (last) {
        if ((rc = stream_flush(c, true))) return rc;
        c->input_done = true;
    }
    return MKT_OK;
}

int mkt_input_window(mkt_ctx* c, char** buf, size_t* cap) {
    if (!c || !buf || !cap) return MKT_E_ARG;
    int rc = stream_check_open(c);
    if (rc) return rc;
    if (c->h_len == c->block_cap) {
        if ((rc = stream_flush(c, false))) return rc;
        if ((rc = stream_alloc_in(c, c->cur))) return rc;
    }
    *buf = (char*)c->in[c->cur].h.get() + c->h_len;
    *cap = c->block_cap - c->h_len;
    return MKT_OK;
}
int mkt_submit_window(mkt_ctx* c, size_t n, int last) {
    if (!c) return MKT_E_ARG;
    if (c->input_done || c->finished) return fail(c, MKT_E_STATE, "submit after the end of input");
    if (!c->in[c->cur].h || n > c->block_cap - c->h_len) return fail(c, MKT_E_ARG, "more bytes than the input window holds");
    HIPCHK(c, hipSetDevice(c->p.device));
    c->h_len += n;
    c->bytes_in += n;
    int rc;
    if (last) {
        if ((rc = stream_flush(c, true))) return rc;
        c->input_done = true;
    } else if (c->h_len == c->block_cap) {
        if ((rc = stream_flush(c, false))) return rc;
    }
    return MKT_OK;
}

// the staging slot of the chunk handed out last goes back to the worker (c->mu held)
static void release_handed(mkt_ctx* c) {
    if (c->handed_valid) {
        if (c->handed.out_slot >= 0) c->outs[c->handed.out_slot].host_busy = false;
        c->handed = mkt_ctx::Chunk();
        c->handed_valid = false;
        c->cv.notify_all();
    }
}
static void chunk_ptrs(mkt_ctx::Chunk& ch) {        // a heap chunk's pointers follow its vectors (they move with the chunk)
    if (ch.out_slot < 0) { ch.pairs = ch.own_pairs.data(); ch.pairs_len = ch.own_pairs.size(); ch.sam = ch.own_sam.data(); ch.sam_len = ch.own_sam.size(); }
}

int mkt_drain(mkt_ctx* c, mkt_out* out) {
    if (!c || !out) return MKT_E_ARG;
    std::unique_lock<std::mutex> lk(c->mu);
    release_handed(c);
    c->drained_pairs.clear(); c->drained_sam.clear();
    while (!c->ready.empty()) {
        mkt_ctx::Chunk& ch = c->ready.front();
        chunk_ptrs(ch);
        c->drained_pairs.insert(c->drained_pairs.end(), ch.pairs, ch.pairs + ch.pairs_len);
        c->drained_sam.insert(c->drained_sam.end(), ch.sam, ch.sam + ch.sam_len);
        if (ch.out_slot >= 0) c->outs[ch.out_slot].host_busy = false;
        c->ready.pop_front();
    }
    c->cv.notify_all();
    out->pairs = c->drained_pairs.data(); out->pairs_len = c->drained_pairs.size();
    out->sam = c->drained_sam.data(); out->sam_len = c->drained_sam.size();
    return c->async_rc;
}

int mkt_drain_wait(mkt_ctx* c, mkt_out* out, int* done) {
    if (!c || !out || !done) return MKT_E_ARG;
    std::unique_lock<std::mutex> lk(c->mu);
    release_handed(c);
    memset(out, 0, sizeof *out);
    *done = 0;
    c->consumer_async = true;
    c->cv.wait(lk, [&] { return c->async_rc != MKT_OK || !c->ready.empty() || c->finished; });
    if (!c->ready.empty()) {
        c->handed = std::move(c->ready.front());
        c->ready.pop_front();
        c->handed_valid = true;
        chunk_ptrs(c->handed);
        out->pairs = c->handed.pairs; out->pairs_len = c->handed.pairs_len; out->sam = c->handed.sam; out->sam_len = c->handed.sam_len;
        return MKT_OK;
    }
    *done = 1;
    return c->async_rc;
}

int mkt_submit_device(mkt_ctx* c, const void* d_text, size_t n) {
    if (!c) return MKT_E_ARG;
    if (c->finished) return fail(c, MKT_E_STATE, "submit after finish");
    if (!d_text && n) return fail(c, MKT_E_ARG, "null device pointer");
    HIPCHK(c, hipSetDevice(c->p.device));
    // The self-circle list must have room for what the blocks in flight may add (their counts are known at the next sync)
    // ... and the first block of an input is a probe: its result (self-circle density, tiles the lean kernel could not
    // take) is looked at before the second block is queued
    const bool probe = c->probing && c->res_used >= 1;
    if (probe || c->res_used == c->res_slots - mkt_ctx::kIn || (size_t)c->acc.sc + sc_estimate(c, c->bytes_unsynced + n) > c->d_sc.cap()) {
        if (getenv("MKT_DEBUG_SYNC")) fprintf(stderr, "submit_device: sync before block (slots %zu/%zu, unsynced %.1f GB, density %.3g /B, list %llu of %zu)\n",
                                              c->res_used, c->res_slots, (double)c->bytes_unsynced / 1e9, c->sc_density, (unsigned long long)c->acc.sc, c->d_sc.cap());
        int rc = mkt_sync(c);
        if (rc) return rc;
        // room for as much again as the run holds now, and for this block at the very least
        if ((rc = ensure_sc_list(c, 2 * (size_t)c->acc.sc + sc_estimate(c, n)))) return rc;
    }
    if (!c->dims_probed) {                                 // the input's line length: newlines of the first MiB, counted on the device
        const double avg = probe_device_lines(c, (const uint8_t*)d_text, n);
        if (avg <= 0 && n) return fail(c, MKT_E_HIP, "line-length probe failed: %s", hipGetErrorString(hipGetLastError()));
        set_dims_from_avg(c, avg);
    }
    c->bytes_unsynced += n;
    const int cfg_used = c->cfg;
    const TileDims dims_used = c->dims;
    int rc = enqueue_block(c, (const uint8_t*)d_text, n, cfg_used, dims_used, c->res_used);
    if (rc) return rc;
    if (c->res_text.size() < c->res_slots) { c->res_text.resize(c->res_slots); c->res_n.resize(c->res_slots); }
    c->res_text[c->res_used] = (const uint8_t*)d_text; c->res_n[c->res_used] = n;
    ++c->res_used;
    c->last_n = n; c->last_dims = dims_used; c->last_text = (const uint8_t*)d_text;
    c->bytes_in += n;
    return MKT_OK;
}

int mkt_sync(mkt_ctx* c) {
    if (!c) return MKT_E_ARG;
    HIPCHK(c, hipSetDevice(c->p.device));
    { std::unique_lock<std::mutex> lk(c->mu); const int arc = stream_wait_idle(c, lk); if (arc) return arc; }
    const bool dbg = getenv("MKT_DEBUG_SYNC") != nullptr;
    auto now = [] { return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now().time_since_epoch()).count(); };
    const double t0 = dbg ? now() : 0;
    HIPCHK(c, hipStreamSynchronize(c->stream));
    const double t1 = dbg ? now() : 0;
    fold_timing(c);
    const double t2 = dbg ? now() : 0;
    int rc = MKT_OK;
    // A block whose line table overflowed (shorter lines than the geometry was chosen for: the first block of an input, or
    // a stream whose read length shrinks on the way) is run again with the next smaller geometry -- together with every
    // block queued behind it, which ran on top of run totals the failed block never advanced.  The texts are still resident.
    bool changed = false;
    int replays = 0;
    for (size_t k = c->res_folded; k < c->res_used; ++k) {
        const BlockResult& r = c->h_res[k];
        if (r.err) {
            if ((r.err & (E_LINE_TABLE | E_OVF_SLOTS)) && c->p.tiles == MKT_TILES_AUTO && c->cfg != CFG_SMALL && replays < 4 && c->res_text.size() > k) {
                ++replays;
                ++c->replays.geometry; c->replays.jobs_rerun += c->res_used - k;
                smaller_geometry(c, c->res_text[k], c->res_n[k]);
                c->last_dims = c->dims;
                changed = true;
                if ((rc = rewind_run(c))) return rc;
                for (size_t j = k; j < c->res_used; ++j) if ((rc = enqueue_block(c, c->res_text[j], c->res_n[j], c->cfg, c->dims, j))) return rc;
                HIPCHK(c, hipStreamSynchronize(c->stream));
                fold_timing(c);
                --k;                                     // look at the same block again
                continue;
            }
            rc = check_result(c, r);                     // fail loudly
            break;
        }
        c->acc.add_block(r); c->tiles_total += r.tiles; c->tiles_deferred += r.pad;
        changed = adapt_geometry(c, r) || changed;
        c->sc_unfolded += r.sc; c->emitted_unfolded += r.emitted;
        ++c->blocks;
    }
    if (c->res_used > c->res_folded) c->probing = changed;  // a new geometry is checked on one block before queueing ahead
    const size_t nres = c->res_used;
    c->res_used = 0; c->res_folded = 0;
    if (rc == MKT_OK) note_sc_density(c);
    if (dbg) fprintf(stderr, "mkt_sync: %zu blocks, wait %.2f ms, timing fold %.2f ms, results %.2f ms\n", nres, t1 - t0, t2 - t1, now() - t2);
    return rc;
}

int mkt_fetch_last_block(mkt_ctx* c, char* pairs, size_t pairs_cap, size_t* pairs_len, char* sam, size_t sam_cap, size_t* sam_len) {
    if (!c) return MKT_E_ARG;
    HIPCHK(c, hipSetDevice(c->p.device));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    // the last folded result is not kept per block; re-read it from the device workspace
    BlockResult r;
    const uint32_t ntiles = num_tiles((uint32_t)c->last_n, c->last_dims.tile ? c->last_dims.tile : c->dims.tile);
    HIPCHK(c, hipMemcpy(&r, BlockWs{c->d_ws, ntiles}.res(), sizeof r, hipMemcpyDeviceToHost));
    if (pairs_len) *pairs_len = (size_t)r.pair_bytes;
    if (sam_len) *sam_len = c->P.write_sam ? (size_t)r.sam_bytes : 0;
    const uint32_t nreg = r.nregions ? r.nregions : 1;
    const size_t prc = (c->d_pairs.cap() / nreg) & ~(size_t)15, src_ = c->P.write_sam ? ((c->d_sam.cap() / nreg) & ~(size_t)15) : 0;
    if (pairs && r.pair_bytes) {
        if (pairs_cap < r.pair_bytes) return fail(c, MKT_E_ARG, "pairs buffer too small (%llu needed)", (unsigned long long)r.pair_bytes);
        size_t acc = 0;
        for (uint32_t q = 0; q < nreg; ++q) { if (r.rpair[q]) HIPCHK(c, hipMemcpy(pairs + acc, c->d_pairs + (size_t)q * prc, (size_t)r.rpair[q], hipMemcpyDeviceToHost)); acc += (size_t)r.rpair[q]; }
    }
    if (sam && c->P.write_sam && r.sam_bytes) {
        if (sam_cap < r.sam_bytes) return fail(c, MKT_E_ARG, "sam buffer too small (%llu needed)", (unsigned long long)r.sam_bytes);
        size_t acc = 0;
        for (uint32_t q = 0; q < nreg; ++q) { if (r.rsam[q]) HIPCHK(c, hipMemcpy(sam + acc, c->d_sam + (size_t)q * src_, (size_t)r.rsam[q], hipMemcpyDeviceToHost)); acc += (size_t)r.rsam[q]; }
    }
    return MKT_OK;
}

int mkt_finish(mkt_ctx* c, int drop_last, uint64_t group_offset, uint64_t total_groups, mkt_stats* st) {
    if (!c || !st) return MKT_E_ARG;
    int rc = mkt_sync(c);
    if (rc) return rc;
    const uint64_t K = total_groups ? total_groups : c->acc.groups;
    unsigned long long logged = 0;
    if (c->acc.sc) {
        if (!c->d_sc_logged) HIPCHK(c, c->d_sc_logged.alloc(1));
        HIPCHK(c, hipMemsetAsync(c->d_sc_logged, 0, sizeof(unsigned long long), c->stream));
        const uint64_t drop_group = c->acc.drops(drop_last != 0) ? c->acc.groups - 1 : ~0ull;
        HIPCHK(c, launch_sc_logged(c->d_sc, c->acc.sc, drop_group, group_offset, K, (uint32_t)c->p.ref_threads, c->d_sc_logged, c->stream));
        HIPCHK(c, hipMemcpyAsync(&logged, c->d_sc_logged, sizeof logged, hipMemcpyDeviceToHost, c->stream));
        HIPCHK(c, hipStreamSynchronize(c->stream));
    }
    RunStats s = c->acc.finish_logged(drop_last != 0, logged);
    memset(st, 0, sizeof *st);
    st->lowMap = s.counters[C_LOWMAP]; st->manyHits = s.counters[C_MANYHITS]; st->unpaired = s.counters[C_UNPAIRED];
    st->selfCircle = s.counters[C_SELFCIRCLE]; st->trans = s.counters[C_TRANS];
    st->cis10K = s.counters[C_CIS10K]; st->cis1K = s.counters[C_CIS1K]; st->cis0 = s.counters[C_CIS0];
    st->selfCircle_all = s.selfcircle_all;
    st->groups = s.groups; st->pairs = s.pairs; st->pair_bytes = s.pair_bytes; st->sam_bytes = s.sam_bytes;
    st->bytes_in = c->bytes_in; st->blocks = c->blocks;
    {
        std::lock_guard<std::mutex> g(c->mu);
        if (!c->finished) {
            if (!drop_last && (!c->tail_pairs.empty() || !c->tail_sam.empty())) {      // the newest group is final after all: release it
                mkt_ctx::Chunk t;
                t.own_pairs.swap(c->tail_pairs); t.own_sam.swap(c->tail_sam);
                c->ready.push_back(std::move(t));
            }
            c->tail_pairs.clear(); c->tail_sam.clear();
            c->finished = true;
        }
    }
    c->cv.notify_all();
    return MKT_OK;
}

int mkt_reset(mkt_ctx* c) {
    if (!c) return MKT_E_ARG;
    HIPCHK(c, hipSetDevice(c->p.device));
    {   // the streaming pipeline idle (an earlier asynchronous error is forgotten with the input it belonged to)
        std::unique_lock<std::mutex> lk(c->mu);
        c->cv.wait(lk, [&] { return c->async_rc != MKT_OK || c->jobs.empty(); });
        (void)sync_all(c);
        c->jobs.clear(); c->ready.clear(); c->handed = mkt_ctx::Chunk(); c->handed_valid = false;
        for (int i = 0; i < mkt_ctx::kIn; ++i) c->in[i].busy = false;
        for (int i = 0; i < mkt_ctx::kOut; ++i) { c->outs[i].dev_busy = false; c->outs[i].host_busy = false; }
        c->async_rc = MKT_OK; c->cur = 0; c->seq = 0; c->consumer_async = false;
    }
    HIPCHK(c, hipStreamSynchronize(c->stream));
    fold_timing(c);
    HIPCHK(c, hipMemsetAsync(c->d_run, 0, sizeof(DevRun), c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    c->acc = RunAccum();
    c->sc_unfolded = 0; c->bytes_unsynced = 0; c->emitted_unfolded = 0;
    // a new input is probed afresh for its densities; the tile geometry learned on the previous input is where its probe
    // starts (a context usually sees one kind of data; a fresh context starts from the largest tiles)
    c->sc_density = 0; c->key_density = 0; c->probing = true;
    c->dims_probed = c->p.tiles != MKT_TILES_AUTO || c->p.ordered || c->cfg == CFG_SMALL;      // a new input: its own line length
    if (c->d_chr) HIPCHK(c, hipMemsetAsync(c->d_chr, 0, sizeof(ChrTab), c->stream));
    c->res_used = c->res_folded = 0;
    c->h_len = 0;
    c->tail_pairs.clear(); c->tail_sam.clear(); c->drained_pairs.clear(); c->drained_sam.clear();
    c->input_done = c->finished = false;
    c->bytes_in = 0; c->blocks = 0;
    return MKT_OK;
}

int mkt_format_log(const mkt_stats* st, char* out, size_t cap) {
    if (!st || !out) return MKT_E_ARG;
    return snprintf(out, cap, "lowMap\t%u\nmanyHits\t%u\nunpaired\t%u\nselfCircle\t%u\ntrans\t%u\ncis10K\t%u\ncis1K\t%u\ncis0\t%u\n",
                    st->lowMap, st->manyHits, st->unpaired, st->selfCircle, st->trans, st->cis10K, st->cis1K, st->cis0);
}

int mkt_get_timing(const mkt_ctx* c, mkt_timing* t) {
    if (!c || !t) return MKT_E_ARG;
    t->tile_kernel_ms = c->folded_ms; t->tile_launches = c->folded_launches; t->tile_bytes = c->folded_bytes; t->other_ms = 0;
    t->tiles = c->tiles_total; t->deferred_tiles = c->tiles_deferred;
    return MKT_OK;
}
int mkt_reset_timing(mkt_ctx* c) {
    if (!c) return MKT_E_ARG;
    c->folded_ms = 0; c->folded_launches = 0; c->folded_bytes = 0; c->tiles_total = 0; c->tiles_deferred = 0;
    std::lock_guard<std::mutex> g(c->mu);
    c->replays = mkt_replays{0, 0, 0, 0, 0};
    return MKT_OK;
}
int mkt_get_replays(const mkt_ctx* c, mkt_replays* r) {
    if (!c || !r) return MKT_E_ARG;
    std::lock_guard<std::mutex> g(const_cast<mkt_ctx*>(c)->mu);       // (the streaming worker counts under the same lock)
    *r = c->replays;
    return MKT_OK;
}

}  // extern "C"
