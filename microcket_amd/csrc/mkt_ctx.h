// mkt_ctx.h -- the context behind include/mkt.h and what the units of the C ABI share (mkt_capi.cpp: blocks and both paths,
// mkt_capi_ext.cpp: the MKT_EXT_KEYS extensions, mkt_capi_util.cpp: generator, data sets, utilities).  Internal: never installed.
// Every device / pinned allocation, event and stream of a context is a member that owns it (mkt_devbuf.h): `delete c` frees them.
#pragma once
#include <hip/hip_runtime.h>
#include <stdarg.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <algorithm>
#include <string>
#include <utility>
#include <chrono>
#include <condition_variable>
#include <deque>
#include <mutex>
#include <thread>
#include <vector>

#include "../../include/mkt.h"
#include "mkt_launch.h"
#include "mkt_devbuf.h"

using namespace mkt;

// block offsets are 32 bit, the ordered kernels pack byte counts into 31-bit fields
static const size_t kMaxBlock = ((size_t)1 << 31) - 65536;
// rounds of the lean kernel's tiles dealt by ticket at the end of a block (profiles/fast_dealing.txt has the sweep); 0: all static
static const uint32_t kFastRoundsDefault = 8;
static const size_t kStampWords = 20;        // diagnostic builds: 16 phase words + 4 span words (mkt_debug_stamps / mkt_debug_spans)

inline thread_local std::string g_create_error;

struct mkt_ctx {
    mkt_params p;
    Params P;
    // the streams come first: they are destroyed last, after every buffer and event
    DevStream stream, s_in, s_out;
    int cfg = CFG_FAST;
    TileDims dims = {0, 0, 0};          // bytes per tile / halos of the blocks to come (MKT_TILES_AUTO: from the input's line length)
    bool dims_probed = false;           // the line length of this input has been looked at
    DevBuf<unsigned long long> d_probe; PinBuf<unsigned long long> h_probe;      // resident path: newline count of the first MiB
    TileDims last_dims = {0, 0, 0};     // geometry of the newest resident block (mkt_fetch_last_block)
    const uint8_t* last_text = nullptr; // its text (valid until the next sync: a failed probe block is re-run)
    bool probing = true;                // the next resident block is looked at before more are queued
    size_t block_cap = 0;
    // device
    GrowBuf<uint8_t> d_pairs, d_sam;
    GrowBuf<uint64_t> d_sc;                               // the run's resolved self-circle list (drained at syncs)
    DevBuf<unsigned long long> d_sc_logged;               // result word of k_sc_logged
    PinBuf<uint8_t> h_chr_stage; DevBuf<uint16_t> d_dense;                    // mkt_ext_chrstat: pinned staging, slot -> dense id
    GrowBuf<uint8_t> d_dd_flags, d_dd_work;               // mkt_ext_dedup
    DevBuf<DedupResult> d_dd_res; PinBuf<DedupResult> h_dd_res;
    GrowBuf<uint32_t> d_perm; DevBuf<uint32_t> d_part_hist; DevBuf<uint16_t> d_lut; uint64_t part_n = 0;      // sharded duplicate marking
    GrowBuf<unsigned long long> d_chr_counts; PinGrowBuf<unsigned long long> h_chr_counts;
    double sc_density = 0;                                // most self-circles per input byte seen between two syncs (0: nothing seen yet)
    GrowBuf<uint64_t> d_sc_tmp;                           // per block: raw (tile, ordinal) entries, one slice per region
    // extensions (MKT_EXT_KEYS)
    GrowBuf<KeyRec> d_keys_raw;                           // per block, one slice per region
    GrowBuf<KeyRec> d_key_list;                           // the run's keys in input order
    DevBuf<ChrTab> d_chr;
    GrowBuf<uint8_t> d_ws;                                // the block workspace (BlockWs)
    DevBuf<DevRun> d_run;
    // host (pinned)
    size_t h_len = 0;                   // bytes in the input slot being filled
    PinBuf<BlockResult> h_res; size_t res_slots = 0, res_used = 0, res_folded = 0;
    std::vector<DevBuf<uint8_t>> uploads; // mkt_device_text buffers (freed with the context)
    std::vector<const uint8_t*> res_text; std::vector<size_t> res_n;      // resident path: the text of every queued block (a failed one is re-run)
    // ---- streaming pipeline (mkt_submit / mkt_input_window): the caller fills pinned input slots and queues GPU work
    // without waiting; one worker thread takes the results in order, copies the outputs back and hands them to the
    // consumer (mkt_drain / mkt_drain_wait).  reader || H2D || kernels || D2H || writer all overlap.
    static constexpr int kIn = 3, kOut = 2;
    static constexpr size_t kHead = 65536;                // room in front of a staged output for the held-back group of the block before
    enum { EV_H2D, EV_K0, EV_K1, EV_DONE };
    struct InSlot { PinBuf<uint8_t> h; DevBuf<uint8_t> d; bool busy = false; DevEvents<4> ev; };
    struct OutSlot { GrowBuf<uint8_t> d_pairs, d_sam; PinGrowBuf<uint8_t> h; bool dev_busy = false, host_busy = false; };
    struct Job { int in_slot, out_slot; size_t n; int cfg; TileDims dims; int attempts; };
    struct Chunk { const char* pairs = nullptr; size_t pairs_len = 0; const char* sam = nullptr; size_t sam_len = 0; int out_slot = -1;
                   std::vector<char> own_pairs, own_sam; };
    InSlot in[kIn];
    OutSlot outs[kOut];
    std::deque<Job> jobs;                                 // queued on the GPU, results not yet taken (front = oldest)
    std::deque<Chunk> ready;                              // final output bytes waiting for the consumer
    Chunk handed; bool handed_valid = false;              // what mkt_drain_wait returned last (its staging slot is released by the next call)
    std::mutex mu;
    std::condition_variable cv;
    std::thread worker;
    bool worker_started = false, stop = false;
    int async_rc = MKT_OK;                                // first error the worker met; every later call reports it
    bool consumer_async = false;                          // mkt_drain_wait in use: another thread takes the outputs, so a full staging slot means WAIT (back-pressure)
    int cur = 0;                                          // input slot the caller is filling
    uint64_t seq = 0;
    std::vector<char> tail_pairs, tail_sam, drained_pairs, drained_sam;
    RunAccum acc;
    bool input_done = false, finished = false;
    uint64_t bytes_in = 0, blocks = 0;
    size_t last_n = 0;                   // bytes of the last resident block
    double key_density = 0;              // extension: most reported pairs per input byte seen between two syncs (0: nothing seen yet)
    uint64_t emitted_unfolded = 0;
    uint64_t sc_unfolded = 0;            // self-circle entries of the blocks folded at the last sync (for the density estimate)
    uint64_t bytes_unsynced = 0;         // resident bytes enqueued since the last sync
    // timing
    struct Timed { DevEvents<2> ev; uint64_t bytes = 0; };
    std::deque<Timed> ev;                // resident path: start / stop of the tile kernel of every block since the last sync
    double folded_ms = 0; uint64_t folded_launches = 0, folded_bytes = 0;
    uint64_t tiles_total = 0, tiles_deferred = 0;      // lean-kernel tiles / those it left to the generic kernel
    mkt_replays replays = {0, 0, 0, 0, 0};             // repairs by cause and blocks run again (streaming: written by the worker under mu)
    // synth
    GrowBuf<char> d_syn;
    GrowBuf<uint64_t> d_syn_sizes;
    DevBuf<unsigned long long> d_stamps;      // diagnostic builds (MKT_STAMPS) only
    uint32_t fast_rounds = kFastRoundsDefault; // lean kernel: rounds of tiles dealt by ticket at the end of a block (MKT_FAST_ROUNDS)
    bool no_lean = false;                     // MKT_NO_LEAN=1: generic kernel only (debugging aid)
    int halo_widened = 0;                     // times adapt_geometry widened the halos of this input (at most twice)
    std::string err;
};

inline int fail(mkt_ctx* c, int code, const char* fmt, ...) {
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    if (c) c->err = buf; else g_create_error = buf;
    return code;
}
#define HIPCHK(c, call)                                                                            \
    do {                                                                                           \
        hipError_t e_ = (call);                                                                    \
        if (e_ != hipSuccess) return fail((c), MKT_E_HIP, "%s failed: %s", #call, hipGetErrorString(e_)); \
    } while (0)

// every stream of the context idle (before a device buffer that queued work may still use is freed)
inline int sync_all(mkt_ctx* c) {
    if (c->s_in) HIPCHK(c, hipStreamSynchronize(c->s_in));
    if (c->stream) HIPCHK(c, hipStreamSynchronize(c->stream));
    if (c->s_out) HIPCHK(c, hipStreamSynchronize(c->s_out));
    return MKT_OK;
}
// room for `need` elements: the buffer as it is, else a new one of new_cap elements (the caller's slack formula), contents dropped.
// sync: work queued on the context may still use the old buffer, so its streams go idle before that is freed.
template <typename B>
inline int ensure(mkt_ctx* c, B& buf, size_t need, size_t new_cap, bool sync) {
    if (buf.fits(need)) return MKT_OK;
    if (sync && buf.get()) { const int rc = sync_all(c); if (rc) return rc; }
    HIPCHK(c, buf.regrow(new_cap));
    return MKT_OK;
}
// the run's key records (quirk Q1: without the one of the input's last group, when that reported a pair)
inline uint64_t ext_key_count(mkt_ctx* c, int drop_last) {
    uint64_t n = c->acc.emitted;
    if (drop_last && c->acc.pending.valid && c->acc.pending.pair_bytes && n) --n;
    return n;
}
