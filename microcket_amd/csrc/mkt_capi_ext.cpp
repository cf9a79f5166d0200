// mkt_capi_ext.cpp -- the MKT_EXT_KEYS extensions of the C ABI over the run's key list: duplicate marking (one context, host keys,
// sharded over the contexts of one process), partition / unpartition for the multi-GPU exchange, per-chromosome counts.
#include "mkt_ctx.h"

extern "C" {

static int ensure_dedup_work(mkt_ctx* c, uint64_t n);
int mkt_ext_dedup(mkt_ctx* c, int drop_last, uint64_t* total, uint64_t* dups, uint8_t* flags, size_t flags_cap) {
    if (!c) return MKT_E_ARG;
    if (!(c->p.extensions & MKT_EXT_KEYS)) return fail(c, MKT_E_STATE, "context created without MKT_EXT_KEYS");
    int rc = mkt_sync(c);
    if (rc) return rc;
    const uint64_t n = ext_key_count(c, drop_last);
    if (total) *total = n;
    if (dups) *dups = 0;
    if (n == 0) return MKT_OK;
    if (flags && flags_cap < n) return fail(c, MKT_E_ARG, "flags buffer too small (%llu needed)", (unsigned long long)n);
    const size_t wb = dedup_work_bytes(n);
    if ((rc = ensure_dedup_work(c, n))) return rc;
    HIPCHK(c, launch_dedup(c->d_key_list, n, c->d_dd_flags, c->d_dd_work.get(), wb, c->d_dd_res, c->stream));
    HIPCHK(c, hipMemcpyAsync(c->h_dd_res, c->d_dd_res, sizeof(DedupResult), hipMemcpyDeviceToHost, c->stream));
    if (flags) HIPCHK(c, hipMemcpyAsync(flags, c->d_dd_flags, n, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    if (dups) *dups = c->h_dd_res->dups;
    return MKT_OK;
}
int mkt_ext_chr_names(mkt_ctx* c, char* out, size_t cap, size_t* len) {
    if (!c || !len) return MKT_E_ARG;
    if (!(c->p.extensions & MKT_EXT_KEYS)) return fail(c, MKT_E_STATE, "context created without MKT_EXT_KEYS");
    int rc = mkt_sync(c);
    if (rc) return rc;
    *len = 0;
    if (!c->d_chr) return MKT_OK;
    std::vector<unsigned long long> hh(kChrSlots);
    std::vector<uint8_t> names((size_t)kChrSlots * 64);
    HIPCHK(c, hipMemcpy(hh.data(), c->d_chr->hash, kChrSlots * sizeof(unsigned long long), hipMemcpyDeviceToHost));
    HIPCHK(c, hipMemcpy(names.data(), c->d_chr->name, names.size(), hipMemcpyDeviceToHost));
    std::string txt;
    char num[16];
    for (uint32_t s2 = 0; s2 < kChrSlots; ++s2) if (hh[s2]) {
        snprintf(num, sizeof num, "%u", s2);
        txt += num; txt += '\t'; txt.append((const char*)&names[(size_t)s2 * 64], names[(size_t)s2 * 64 + 63]); txt += '\n';
    }
    *len = txt.size();
    if (out) { if (cap < txt.size()) return fail(c, MKT_E_ARG, "buffer too small (%zu needed)", txt.size()); memcpy(out, txt.data(), txt.size()); }
    return MKT_OK;
}
int mkt_ext_keys_fetch(mkt_ctx* c, int drop_last, void* keys, size_t cap_bytes, uint64_t* n) {
    if (!c || !n) return MKT_E_ARG;
    if (!(c->p.extensions & MKT_EXT_KEYS)) return fail(c, MKT_E_STATE, "context created without MKT_EXT_KEYS");
    int rc = mkt_sync(c);
    if (rc) return rc;
    *n = ext_key_count(c, drop_last);
    if (keys && *n) {
        if (cap_bytes < *n * sizeof(KeyRec)) return fail(c, MKT_E_ARG, "key buffer too small (%llu bytes needed)", (unsigned long long)(*n * sizeof(KeyRec)));
        HIPCHK(c, hipMemcpy(keys, c->d_key_list, (size_t)*n * sizeof(KeyRec), hipMemcpyDeviceToHost));
    }
    return MKT_OK;
}
// work buffers of the duplicate marking, kept between calls (GB-sized hipMalloc / hipFree pairs cost more than the marking)
static int ensure_dedup_work(mkt_ctx* c, uint64_t n) {
    const size_t wb = dedup_work_bytes(n);
    int rc;
    if ((rc = ensure(c, c->d_dd_flags, n, n + n / 8 + 4096, false))) return rc;
    if ((rc = ensure(c, c->d_dd_work, wb, wb + wb / 8, false))) return rc;
    if (!c->h_dd_res) { HIPCHK(c, c->d_dd_res.alloc(1)); HIPCHK(c, c->h_dd_res.alloc(1)); }
    return MKT_OK;
}
int mkt_ext_dedup_device(mkt_ctx* c, const void* d_keys, uint64_t n, uint8_t* d_flags, uint64_t* dups) {
    if (!c || (n && (!d_keys || !d_flags))) return MKT_E_ARG;
    HIPCHK(c, hipSetDevice(c->p.device));
    if (dups) *dups = 0;
    if (n == 0) return MKT_OK;
    int rc = ensure_dedup_work(c, n);
    if (rc) return rc;
    HIPCHK(c, launch_dedup((const KeyRec*)d_keys, n, d_flags, c->d_dd_work.get(), dedup_work_bytes(n), c->d_dd_res, c->stream));
    HIPCHK(c, hipMemcpyAsync(c->h_dd_res, c->d_dd_res, sizeof(DedupResult), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    if (dups) *dups = c->h_dd_res->dups;
    return MKT_OK;
}
int mkt_ext_dedup_keys(mkt_ctx* c, const void* keys, uint64_t n, uint8_t* flags, uint64_t* dups) {
    if (!c || (n && (!keys || !flags))) return MKT_E_ARG;
    HIPCHK(c, hipSetDevice(c->p.device));
    if (dups) *dups = 0;
    if (n == 0) return MKT_OK;
    int rc = ensure_dedup_work(c, n);
    if (rc) return rc;
    DevBuf<KeyRec> d_keys;                                   // (released behind the synchronisation, on every path)
    HIPCHK(c, d_keys.alloc((size_t)n));
    hipError_t e = hipMemcpyAsync(d_keys, keys, (size_t)n * sizeof(KeyRec), hipMemcpyHostToDevice, c->stream);
    if (e == hipSuccess) e = launch_dedup(d_keys, n, c->d_dd_flags, c->d_dd_work.get(), dedup_work_bytes(n), c->d_dd_res, c->stream);
    if (e == hipSuccess) e = hipMemcpyAsync(c->h_dd_res, c->d_dd_res, sizeof(DedupResult), hipMemcpyDeviceToHost, c->stream);
    if (e == hipSuccess) e = hipMemcpyAsync(flags, c->d_dd_flags, n, hipMemcpyDeviceToHost, c->stream);
    const hipError_t e2 = hipStreamSynchronize(c->stream);
    if (e != hipSuccess || e2 != hipSuccess) return fail(c, MKT_E_HIP, "duplicate marking of %llu host keys failed: %s", (unsigned long long)n, hipGetErrorString(e != hipSuccess ? e : e2));
    if (dups) *dups = c->h_dd_res->dups;
    return MKT_OK;
}
int mkt_ext_keys_device(mkt_ctx* c, int drop_last, const void** d_keys, uint64_t* n) {
    if (!c || !d_keys || !n) return MKT_E_ARG;
    if (!(c->p.extensions & MKT_EXT_KEYS)) return fail(c, MKT_E_STATE, "context created without MKT_EXT_KEYS");
    int rc = mkt_sync(c);
    if (rc) return rc;
    *n = ext_key_count(c, drop_last);
    *d_keys = c->d_key_list;
    return MKT_OK;
}
int mkt_ext_partition(mkt_ctx* c, int drop_last, const uint16_t* lut, uint32_t world, void* d_send, uint64_t* counts) {
    if (!c || !counts || world == 0 || world > 16) return MKT_E_ARG;
    if (!(c->p.extensions & MKT_EXT_KEYS)) return fail(c, MKT_E_STATE, "context created without MKT_EXT_KEYS");
    int rc = mkt_sync(c);
    if (rc) return rc;
    const uint64_t n = ext_key_count(c, drop_last);
    for (uint32_t d = 0; d < world; ++d) counts[d] = 0;
    c->part_n = n;
    if (n == 0) return MKT_OK;
    if (!d_send) return MKT_E_ARG;
    if ((rc = ensure(c, c->d_perm, n, n + n / 8 + 1024, false))) return rc;
    if (!c->d_part_hist) HIPCHK(c, c->d_part_hist.alloc(0, partition_work_bytes()));
    if (lut) {
        if (!c->d_lut) HIPCHK(c, c->d_lut.alloc(kChrSlots));
        HIPCHK(c, hipMemcpyAsync(c->d_lut, lut, kChrSlots * sizeof(uint16_t), hipMemcpyHostToDevice, c->stream));
    }
    uint32_t G = 1;
    HIPCHK(c, launch_partition(c->d_key_list, n, lut ? c->d_lut.get() : nullptr, world, c->d_part_hist, (KeyRec*)d_send, c->d_perm, &G, c->stream));
    std::vector<uint32_t> hh((size_t)16 * G);
    HIPCHK(c, hipMemcpyAsync(hh.data(), c->d_part_hist, hh.size() * sizeof(uint32_t), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    for (uint32_t d = 0; d < world; ++d) {
        const uint64_t lo = hh[(size_t)d * G], hi = d + 1 < 16 ? hh[(size_t)(d + 1) * G] : n;      // starts of the destinations in `send` (exclusive scan)
        counts[d] = (d + 1 < world ? hi : n) - lo;
    }
    return MKT_OK;
}
int mkt_ext_unpartition(mkt_ctx* c, const uint8_t* d_flags_part, uint8_t* flags, size_t flags_cap, uint64_t* dups) {
    if (!c) return MKT_E_ARG;
    HIPCHK(c, hipSetDevice(c->p.device));
    const uint64_t n = c->part_n;
    if (dups) *dups = 0;
    if (n == 0) return MKT_OK;
    if (!d_flags_part || !c->d_perm) return MKT_E_ARG;
    if (flags && flags_cap < n) return fail(c, MKT_E_ARG, "flags buffer too small (%llu needed)", (unsigned long long)n);
    int rc = ensure_dedup_work(c, n);
    if (rc) return rc;
    HIPCHK(c, launch_unpermute(d_flags_part, c->d_perm, n, c->d_dd_flags, (unsigned long long*)&c->d_dd_res->dups, c->stream));
    HIPCHK(c, hipMemcpyAsync(c->h_dd_res, c->d_dd_res, sizeof(DedupResult), hipMemcpyDeviceToHost, c->stream));
    if (flags) HIPCHK(c, hipMemcpyAsync(flags, c->d_dd_flags, n, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    if (dups) *dups = c->h_dd_res->dups;
    return MKT_OK;
}
// Duplicate marking across the contexts of ONE process (one context per GPU, contiguous shards of the input in rank order): the
// in-process form of microcket_amd/shard.py's exchange.  Every key record travels to the context mix64(key) % world -- device to
// device, hipMemcpyPeerAsync: between two GPUs of one node that is one xGMI hop, nothing passes through the host --, is marked
// there together with the equal keys of all other shards (segments are laid down in source-rank order and the partition is
// stable, so "first in input order wins" holds globally), and one byte per record travels back the same way.
int mkt_ext_dedup_multi(mkt_ctx** cs, uint32_t world, uint32_t last_rank, uint64_t* totals, uint64_t* dups, uint8_t** flags, const size_t* flags_cap) {
    if (!cs || world == 0 || world > 16 || !totals || !dups) return MKT_E_ARG;
    for (uint32_t r = 0; r < world; ++r) {
        if (!cs[r]) return MKT_E_ARG;
        if (!(cs[r]->p.extensions & MKT_EXT_KEYS)) return fail(cs[r], MKT_E_STATE, "context created without MKT_EXT_KEYS");
        if ((cs[r]->p.extensions ^ cs[0]->p.extensions) & MKT_EXT_LANES) return fail(cs[r], MKT_E_ARG, "contexts disagree on MKT_EXT_LANES");
    }
    mkt_ctx* c0 = cs[0];
    // chromosome slots are per context: every slot -> the rank of its name in the sorted union of all tables
    std::vector<std::vector<std::pair<uint32_t, std::string>>> tabs(world);
    std::vector<std::string> uni;
    for (uint32_t r = 0; r < world; ++r) {
        size_t len = 0;
        int rc = mkt_ext_chr_names(cs[r], nullptr, 0, &len);
        if (rc) return rc;
        std::string txt(len, '\0');
        if (len && (rc = mkt_ext_chr_names(cs[r], &txt[0], len, &len))) return rc;
        size_t p0 = 0;
        while (p0 < txt.size()) {
            const size_t nl = txt.find('\n', p0), tb = txt.find('\t', p0);
            if (nl == std::string::npos || tb == std::string::npos || tb > nl) break;
            tabs[r].push_back({(uint32_t)atoi(txt.substr(p0, tb - p0).c_str()), txt.substr(tb + 1, nl - tb - 1)});
            uni.push_back(tabs[r].back().second);
            p0 = nl + 1;
        }
    }
    std::sort(uni.begin(), uni.end());
    uni.erase(std::unique(uni.begin(), uni.end()), uni.end());
    if (uni.size() > kChrSlots) return fail(c0, MKT_E_CAPACITY, "more than %u chromosome names over all shards", kChrSlots);
    // what rank r holds for the exchange; it is freed with r's device current
    struct Side {
        int device = 0;
        DevBuf<uint8_t> d_send, d_recv, d_flags, d_back;
        uint64_t n = 0, nrecv = 0; uint64_t cnt[16];
        ~Side() { (void)hipSetDevice(device); }
    };
    std::vector<Side> sd(world);
    for (uint32_t r = 0; r < world; ++r) sd[r].device = cs[r]->p.device;
    // partition every shard's keys by destination (stable), slots rewritten to the shared ids
    for (uint32_t r = 0; r < world; ++r) {
        mkt_ctx* c = cs[r];
        std::vector<uint16_t> lut(kChrSlots, 0);
        for (const auto& e : tabs[r]) lut[e.first & (kChrSlots - 1)] = (uint16_t)(std::lower_bound(uni.begin(), uni.end(), e.second) - uni.begin());
        int rc = mkt_sync(c);
        if (rc) return rc;
        sd[r].n = ext_key_count(c, r == last_rank);
        totals[r] = sd[r].n;
        for (uint32_t d = 0; d < 16; ++d) sd[r].cnt[d] = 0;
        if (sd[r].n) HIPCHK(c, sd[r].d_send.alloc((size_t)sd[r].n * sizeof(KeyRec)));
        rc = mkt_ext_partition(c, r == last_rank, lut.data(), world, sd[r].d_send, sd[r].cnt);
        if (rc) return rc;
    }
    for (uint32_t a = 0; a < world; ++a)                         // direct device-to-device copies where the hardware offers them (best effort)
        for (uint32_t b = 0; b < world; ++b)
            if (cs[a]->p.device != cs[b]->p.device) {
                int can = 0;
                if (hipDeviceCanAccessPeer(&can, cs[a]->p.device, cs[b]->p.device) == hipSuccess && can) {
                    (void)hipSetDevice(cs[a]->p.device);
                    const hipError_t e = hipDeviceEnablePeerAccess(cs[b]->p.device, 0);
                    if (e != hipSuccess) (void)hipGetLastError();      // (already enabled: fine)
                }
            }
    // the exchange: rank r receives, in source-rank order, what every rank s partitioned for it
    for (uint32_t r = 0; r < world; ++r) {
        mkt_ctx* c = cs[r];
        HIPCHK(c, hipSetDevice(c->p.device));
        sd[r].nrecv = 0;
        for (uint32_t s2 = 0; s2 < world; ++s2) sd[r].nrecv += sd[s2].cnt[r];
        if (!sd[r].nrecv) continue;
        HIPCHK(c, sd[r].d_recv.alloc((size_t)sd[r].nrecv * sizeof(KeyRec)));
        HIPCHK(c, sd[r].d_flags.alloc((size_t)sd[r].nrecv));
        uint64_t at = 0;
        for (uint32_t s2 = 0; s2 < world; ++s2) {
            uint64_t soff = 0;
            for (uint32_t d = 0; d < r; ++d) soff += sd[s2].cnt[d];
            const uint64_t k = sd[s2].cnt[r];
            if (k) HIPCHK(c, hipMemcpyPeerAsync(sd[r].d_recv + at * sizeof(KeyRec), c->p.device, sd[s2].d_send + soff * sizeof(KeyRec), cs[s2]->p.device, (size_t)k * sizeof(KeyRec), c->stream));
            at += k;
        }
    }
    uint64_t all_dups = 0;
    for (uint32_t r = 0; r < world; ++r) {
        mkt_ctx* c = cs[r];
        HIPCHK(c, hipSetDevice(c->p.device));
        HIPCHK(c, hipStreamSynchronize(c->stream));
        uint64_t d = 0;
        const int rc = mkt_ext_dedup_device(c, sd[r].d_recv, sd[r].nrecv, sd[r].d_flags, &d);
        if (rc) return rc;
        all_dups += d;
    }
    // one byte per record back to where the record came from
    for (uint32_t s2 = 0; s2 < world; ++s2) {
        mkt_ctx* c = cs[s2];
        HIPCHK(c, hipSetDevice(c->p.device));
        if (!sd[s2].n) { dups[s2] = 0; continue; }
        HIPCHK(c, sd[s2].d_back.alloc((size_t)sd[s2].n));
        uint64_t soff = 0;
        for (uint32_t r = 0; r < world; ++r) {
            uint64_t roff = 0;
            for (uint32_t q = 0; q < s2; ++q) roff += sd[q].cnt[r];
            const uint64_t k = sd[s2].cnt[r];
            if (k) HIPCHK(c, hipMemcpyPeerAsync(sd[s2].d_back + soff, c->p.device, sd[r].d_flags + roff, cs[r]->p.device, (size_t)k, c->stream));
            soff += k;
        }
        HIPCHK(c, hipStreamSynchronize(c->stream));
        const int rc = mkt_ext_unpartition(c, sd[s2].d_back, flags ? flags[s2] : nullptr, flags_cap ? flags_cap[s2] : 0, &dups[s2]);
        if (rc) return rc;
    }
    uint64_t sum = 0;
    for (uint32_t r = 0; r < world; ++r) sum += dups[r];
    if (sum != all_dups) return fail(c0, MKT_E_KERNEL, "duplicate counts disagree after the exchange (%llu marked, %llu returned)", (unsigned long long)all_dups, (unsigned long long)sum);
    return MKT_OK;
}
int mkt_ext_chrstat(mkt_ctx* c, int drop_last, char* out, size_t cap, size_t* len) {
    if (!c || !len) return MKT_E_ARG;
    if (!(c->p.extensions & MKT_EXT_KEYS)) return fail(c, MKT_E_STATE, "context created without MKT_EXT_KEYS");
    int rc = mkt_sync(c);
    if (rc) return rc;
    *len = 0;
    const uint64_t n = ext_key_count(c, drop_last);
    if (n == 0 || !c->d_chr) return MKT_OK;
    // the name table -> dense ids in bytewise name order (through pinned staging: pageable copies cost milliseconds each)
    const size_t name_bytes = (size_t)kChrSlots * 64, hash_bytes = kChrSlots * sizeof(unsigned long long);
    if (!c->h_chr_stage) HIPCHK(c, c->h_chr_stage.alloc(hash_bytes + name_bytes + kChrSlots * sizeof(uint16_t)));
    unsigned long long* hh = (unsigned long long*)c->h_chr_stage.get();
    uint8_t* names = c->h_chr_stage + hash_bytes;
    uint16_t* dense = (uint16_t*)(c->h_chr_stage + hash_bytes + name_bytes);
    HIPCHK(c, hipMemcpyAsync(hh, c->d_chr->hash, hash_bytes, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipMemcpyAsync(names, c->d_chr->name, name_bytes, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    std::vector<std::pair<std::string, uint32_t>> used;
    for (uint32_t s2 = 0; s2 < kChrSlots; ++s2) if (hh[s2]) used.emplace_back(std::string((const char*)&names[(size_t)s2 * 64], names[(size_t)s2 * 64 + 63]), s2);
    std::sort(used.begin(), used.end());
    const uint32_t nd = (uint32_t)used.size();
    memset(dense, 0, kChrSlots * sizeof(uint16_t));
    for (uint32_t d = 0; d < nd; ++d) dense[used[d].second] = (uint16_t)d;
    const size_t cells = (size_t)nd * nd, cnt_bytes = cells * sizeof(unsigned long long);
    if (!c->d_dense) HIPCHK(c, c->d_dense.alloc(kChrSlots));
    if ((rc = ensure(c, c->d_chr_counts, cells, cells, false)) || (rc = ensure(c, c->h_chr_counts, cells, cells, false))) return rc;
    HIPCHK(c, hipMemcpyAsync(c->d_dense, dense, kChrSlots * sizeof(uint16_t), hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipMemsetAsync(c->d_chr_counts, 0, cnt_bytes, c->stream));
    HIPCHK(c, launch_chrstat(c->d_key_list, n, c->d_dense, nd, c->d_chr_counts, c->stream));
    HIPCHK(c, hipMemcpyAsync(c->h_chr_counts, c->d_chr_counts, cnt_bytes, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    const unsigned long long* counts = c->h_chr_counts;
    std::string txt;
    char num[32];
    for (uint32_t a2 = 0; a2 < nd; ++a2)
        for (uint32_t b2 = 0; b2 < nd; ++b2)
            if (counts[(size_t)a2 * nd + b2]) {
                snprintf(num, sizeof num, "%llu", counts[(size_t)a2 * nd + b2]);
                txt += used[a2].first; txt += '\t'; txt += used[b2].first; txt += '\t'; txt += num; txt += '\n';
            }
    *len = txt.size();
    if (out) { if (cap < txt.size()) return fail(c, MKT_E_ARG, "chrstat buffer too small (%zu needed)", txt.size()); memcpy(out, txt.data(), txt.size()); }
    return MKT_OK;
}

}  // extern "C"
