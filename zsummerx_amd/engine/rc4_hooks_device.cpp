// rc4_hooks_device.cpp -- the gfx950 Rc4Hooks (include/zsummerx_amd/rc4_hooks.h)
// over the C-ABI of libzrc4.so (include/zrc4.h).
//
// Memory ("pinned SessionBlock pool"): every SessionBlock
// slab is pinned host memory (hipHostMalloc) that the kernels read and write
// in place -- no staging copies and no per-session calls.  The batch tables
// (slot ids, offsets, lengths, keys) are pinned too.  Payload addressing:
// kernels take one base pointer and 64-bit per-entry offsets; the base is the
// first pinned allocation and an entry's offset is its address minus the base
// in two's complement, so slabs anywhere in the address space share one launch.
//
// Every crypt launch is a zrc4_crypt_grouped_declared batch and every refill a
// zrc4_keystream_grouped one (the groups built here are declared with both):
// entries sorted by slot, one
// 256-entry bucket per 256-slot group touched, so each bucket moves its
// group's S-boxes as one coalesced 64 KiB image whatever subset of the group
// the iteration touches (the kIds gather path is never used here).  The
// out-of-place spans of cryptBatch (one shared plaintext for many sessions)
// are a zrc4_crypt_to_grouped batch of the same layout.
//
// Two modes:
//   direct     one grouped launch per engine iteration over the spans
//              themselves, then a wait.  A span's latency is its serial RC4
//              chain: ~40 ns per byte on one lane (rc4_encryption.h:83-88 is
//              byte-serial), so small batches wait on the chain.
//   reservoir  (default) each slot's keystream is generated AHEAD by the GPU
//              -- a background stream runs zrc4_keystream_grouped -- into a
//              ring of `ring` bytes in PINNED HOST memory (written over PCIe
//              by the kernel; nothing crosses the link the other way).  The
//              hook XORs each span with committed ring bytes on the host: no
//              GPU round trip on the latency path.  Only the tail of a span
//              that its slot's committed keystream does not cover goes to the
//              GPU synchronously.  The wire bytes are the reference's.
// The levels, rings, hungry list and refill queue are the reservoir core's
// (csrc/zrc4_reservoir.hpp, shared with the C-ABI reservoir zrc4_ks_*): its
// header states the design and its invariants.  What the hooks add (streams:
// A = synchronous work, B = background refill):
//   * kernels that touch slot state never run on A and B at once: A waits
//     for every queued refill on B before a seed (flushSeeds) or a tail crypt;
//   * the adaptive switch to direct launches (updateMode), the host XOR spread
//     over worker threads (XorPool), the ZSX_* knobs ($ZSX_RING_POISON=1 fills
//     fresh ring slabs with 0xA5) and stats();
//   * the fault latch is polled once after every batch of committed refills.
#include <hip/hip_runtime_api.h>

#include <algorithm>
#include <atomic>
#include <condition_variable>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <new>
#include <mutex>
#include <stdexcept>
#include <string>
#include <thread>
#include <vector>

#include "zrc4.h"
#include "zrc4_reservoir.hpp"
#include "zsummerx_amd/rc4_hooks.h"

namespace zsummerx_amd {
namespace {

// Pinned host allocations shared with the kernels (blocks, rings, batch
// tables) are COHERENT (fine-grained).  HIP dispatches kernels with
// agent-scope acquire/release, so a kernel can hit lines of NON-coherent host
// memory still held in the GPU L2 from an earlier kernel after the host has
// rewritten them (stale batch tables, SessionBlocks, zeroed ring bytes): the
// hooks_check run at 2 048 sessions failed that way with hipHostMallocDefault
// (profiles/r02/hooks_diag.jsonl).  Diagnostic knob:
// ZSX_HOST_ALLOC=coherent|noncoherent|default.
unsigned hostAllocFlags()
{
    static const unsigned f = [] {
        const char *e = std::getenv("ZSX_HOST_ALLOC");
        if (!e) return (unsigned)hipHostMallocCoherent;
        if (!std::strcmp(e, "default")) return (unsigned)hipHostMallocDefault;
        if (!std::strcmp(e, "coherent")) return (unsigned)hipHostMallocCoherent;
        if (!std::strcmp(e, "noncoherent")) return (unsigned)hipHostMallocNonCoherent;
        return (unsigned)hipHostMallocCoherent;
    }();
    return f;
}

// Out of pinned memory is std::bad_alloc here.
template <class T>
struct PinnedArray : zrc4::Pinned<T> {
    void reserve(size_t n)
    {
        if (!zrc4::Pinned<T>::reserve(n, hostAllocFlags())) throw std::bad_alloc();
    }
};

using Table = zrc4::GroupedTable;   // one grouped batch table (ids / offsets / lengths) in pinned memory

// A grouped launch over table t: the groups built here are declared with it
// up to 256 buckets, where the kernels take them in their arguments and load
// each bucket's state with its entries; above that the persistent kernel
// prefetches every bucket's ids a bucket ahead anyway, and a declaration
// would only add the library's up-front check (include/zrc4.h).
int launchGrouped(zrc4_ctx *ctx, const Table &t, uint8_t *base, const zrc4_frame_args *fa, hipStream_t s)
{
    if (t.groups.size() <= 256u)
        return zrc4_crypt_grouped_declared(ctx, t.ids.p, t.groups.data(), base, t.off.p, t.len.p, t.n, fa, s);
    return fa ? zrc4_crypt_grouped_frame(ctx, t.ids.p, base, t.off.p, t.len.p, t.n, fa, s)
              : zrc4_crypt_grouped(ctx, t.ids.p, base, t.off.p, t.len.p, t.n, s);
}

// A refill over table t: the write-only launch (every span receives its
// slot's next keystream bytes, whatever it held), groups declared as above.
int launchKeystream(zrc4_ctx *ctx, const Table &t, uint8_t *base, hipStream_t s)
{
    return zrc4_keystream_grouped(ctx, t.ids.p, t.groups.size() <= 256u ? t.groups.data() : nullptr, base, t.off.p,
                                  t.len.p, t.n, s);
}

// The out-of-place launch of cryptBatch over table t (its off = the
// destinations) with the sources' offsets in soff, declared as launchGrouped
// declares.  Above one bucket per CU the library makes it a copy launch and the
// in-place crypt (include/zrc4.h).
int launchTo(zrc4_ctx *ctx, const Table &t, const uint64_t *soff, uint8_t *base, hipStream_t s)
{
    return zrc4_crypt_to_grouped(ctx, t.ids.p, t.groups.size() <= 256u ? t.groups.data() : nullptr, base, soff, base,
                                 t.off.p, t.len.p, t.n, s);
}

struct Entry {
    uint32_t slot;
    uint32_t len;
    uint64_t off;
    uint32_t idx = 0;     // the caller's span index (framed calls)
    uint32_t flen = 0;    // frame block length (framed calls)
    uint64_t foff = 0;    // frame block offset from the base (framed calls)
    uint64_t soff = 0;    // source offset from the base (out-of-place entries)
};

// Per-entry framing tables of a framed grouped launch (pinned).
struct FrameTable {
    PinnedArray<uint64_t> off;
    PinnedArray<uint32_t> len, npk, used, status, pkt;
    std::vector<int64_t> idx;   // batch entry -> span index (-1: padding)
    void reserve(size_t n)
    {
        off.reserve(n);
        len.reserve(n);
        npk.reserve(n);
        used.reserve(n);
        status.reserve(n);
        pkt.reserve(n * Rc4Frame::kMaxPackets);
    }
};

// The grouped layout of the core's builder over `es`, with the per-entry
// framing tables of a framed launch riding on it.
void buildGrouped(Table &t, std::vector<Entry> &es, FrameTable *ft = nullptr)
{
    if (ft) ft->idx.clear();
    const bool ok = zrc4::buildGrouped(t, es, [&](const Entry *e) {
        if (ft) {
            ft->reserve(t.n);
            ft->off.p[t.n - 1] = e ? e->foff : 0;
            ft->len.p[t.n - 1] = e ? e->flen : 0;
            ft->idx.push_back(e ? (int64_t)e->idx : -1);
        }
    });
    if (!ok) throw std::bad_alloc();
}

// dst ^= src for n bytes (word-wise where possible).
void xorBytes(uint8_t *__restrict dst, const uint8_t *__restrict src, size_t n)
{
    size_t i = 0;
    for (; i + 8 <= n; i += 8) {
        uint64_t a, b;
        std::memcpy(&a, dst + i, 8);
        std::memcpy(&b, src + i, 8);
        a ^= b;
        std::memcpy(dst + i, &a, 8);
    }
    for (; i < n; ++i) dst[i] ^= src[i];
}

// dst = in ^ src for n bytes (dst is only written: it overlaps neither).
void xorBytesTo(uint8_t *__restrict dst, const uint8_t *__restrict in, const uint8_t *__restrict src, size_t n)
{
    size_t i = 0;
    for (; i + 8 <= n; i += 8) {
        uint64_t a, b;
        std::memcpy(&a, in + i, 8);
        std::memcpy(&b, src + i, 8);
        a ^= b;
        std::memcpy(dst + i, &a, 8);
    }
    for (; i < n; ++i) dst[i] = in[i] ^ src[i];
}

// One piece of a reservoir call's host work: span bytes ^= committed ring
// bytes, or with `in` (an out-of-place span) dst = in ^ committed ring bytes.
struct XorJob {
    uint8_t *dst;
    const uint8_t *src;
    uint32_t n;
    const uint8_t *in = nullptr;
    void run() const
    {
        if (in) xorBytesTo(dst, in, src, n);
        else xorBytes(dst, src, n);
    }
};

// The reservoir's host XOR for large batches, spread over worker threads.
// At 2 048 sessions x 2 in flight one call XORs 4 MiB (4 096 spans) and the
// event loop spends ~1 ms in it on one core (profiles/r02/frame_loopback_v2.jsonl:
// 975 us per call, slower than the direct GPU path).  Only the keystream XOR
// is parallel: keystream generation stays on the GPU, and every piece of
// bookkeeping stays on the calling thread.  Threads: $ZSX_XOR_THREADS
// (default min(4, hardware threads / 2); 0 or 1 = inline); batches under
// $ZSX_XOR_MIN_BYTES (default kParallelBytes) run inline.
class XorPool {
public:
    static constexpr size_t kParallelBytes = 256u << 10;

    XorPool()
    {
        if (const char *m = std::getenv("ZSX_XOR_MIN_BYTES")) minBytes_ = (size_t)std::strtoull(m, nullptr, 10);
        const char *e = std::getenv("ZSX_XOR_THREADS");
        unsigned hw = std::thread::hardware_concurrency();
        unsigned t = e ? (unsigned)std::atoi(e) : std::min(4u, hw / 2u);
        workers_ = t > 1u ? t - 1u : 0u;          // the calling thread is one of them
        for (unsigned i = 0; i < workers_; ++i) threads_.emplace_back([this, i] { loop(i + 1u); });
    }
    ~XorPool()
    {
        {
            std::lock_guard<std::mutex> g(mu_);
            stop_ = true;
            ++gen_;
        }
        cv_.notify_all();
        for (std::thread &t : threads_) t.join();
    }
    unsigned threads() const { return workers_ + 1u; }

    void run(const std::vector<XorJob> &jobs, size_t bytes)
    {
        if (!workers_ || bytes < minBytes_ || jobs.size() < 2) {
            for (const XorJob &j : jobs) j.run();
            return;
        }
        // contiguous job ranges of about equal bytes, one per thread
        const unsigned parts = workers_ + 1u;
        bounds_.assign(parts + 1u, jobs.size());
        bounds_[0] = 0;
        size_t acc = 0, k = 1;
        for (size_t i = 0; i < jobs.size() && k < parts; ++i) {
            acc += jobs[i].n;
            if (acc * parts >= bytes * k) bounds_[k++] = i + 1;
        }
        jobs_ = &jobs;
        pending_.store(workers_, std::memory_order_relaxed);
        {
            std::lock_guard<std::mutex> g(mu_);
            ++gen_;
        }
        cv_.notify_all();
        work(0);
        while (pending_.load(std::memory_order_acquire) != 0) std::this_thread::yield();
    }

private:
    void work(unsigned part)
    {
        const std::vector<XorJob> &jobs = *jobs_;
        for (size_t i = bounds_[part]; i < bounds_[part + 1]; ++i) jobs[i].run();
    }
    void loop(unsigned part)
    {
        uint64_t seen = 0;
        for (;;) {
            {
                std::unique_lock<std::mutex> l(mu_);
                cv_.wait(l, [&] { return gen_ != seen; });
                seen = gen_;
                if (stop_) return;
            }
            work(part);
            pending_.fetch_sub(1, std::memory_order_release);
        }
    }
    unsigned workers_ = 0;
    size_t minBytes_ = kParallelBytes;
    std::vector<std::thread> threads_;
    std::mutex mu_;
    std::condition_variable cv_;
    uint64_t gen_ = 0;
    bool stop_ = false;
    const std::vector<XorJob> *jobs_ = nullptr;
    std::vector<size_t> bounds_;
    std::atomic<unsigned> pending_{0};
};

class DeviceRc4Hooks final : public Rc4Hooks {
public:
    DeviceRc4Hooks(int device, uint32_t capacity, uint32_t ringBytes) : ringCap_(ringBytes)
    {
        const int rc = zrc4_create(&ctx_, device, capacity);
        if (rc != ZRC4_OK)
            throw std::runtime_error(std::string("makeDeviceRc4Hooks: zrc4_create: ") + zrc4_strerror(rc));
        bool ok = hipSetDevice(device) == hipSuccess &&
                  hipStreamCreateWithFlags(&sA_, hipStreamNonBlocking) == hipSuccess &&
                  hipStreamCreateWithFlags(&sB_, hipStreamNonBlocking) == hipSuccess;
        tt_.flags = to_.flags = hostAllocFlags();
        if (ok && ringCap_) {
            // $ZSX_REFILL_CHUNK (A/B knob): bytes per slot per refill, at most a
            // quarter of the ring (two refills in flight leave half of it readable)
            const char *rc = std::getenv("ZSX_REFILL_CHUNK");
            const uint32_t want = rc ? (uint32_t)std::strtoul(rc, nullptr, 10) : kRefillChunk;
            refillChunk_ = std::max<uint32_t>(256u, std::min<uint32_t>(want, ringCap_ / 4));
            ok = res_.init(zrc4_capacity(ctx_), ringCap_, refillChunk_, refillDepth_, sB_, hostAllocFlags(),
                           ringPoison_ ? 0xA5 : -1) == ZRC4_OK;
        }
        if (!ok) {
            release();
            throw std::runtime_error("makeDeviceRc4Hooks: HIP stream/event creation failed");
        }
        seen_.assign(zrc4_capacity(ctx_), 0u);
        seenTo_.assign(zrc4_capacity(ctx_), 0u);
    }
    ~DeviceRc4Hooks() override { release(); }

    const char *name() const override { return ringCap_ ? "zrc4-gfx950" : "zrc4-gfx950-direct"; }
    uint32_t capacity() const override { return zrc4_capacity(ctx_); }

    void *allocBlocks(size_t bytes) override
    {
        void *p = nullptr;
        if (hipHostMalloc(&p, bytes, hostAllocFlags()) != hipSuccess) throw std::bad_alloc();
        if (!res_.base) res_.base = static_cast<uint8_t *>(p);
        return p;
    }
    void freeBlocks(void *p) override
    {
        if (p) (void)hipHostFree(p);
    }

    int seed(const uint32_t *slots, uint32_t n, const std::string &key) override
    {
        // Only the first 256 key bytes reach the S-box (rc4_encryption.h:60-70).
        const uint32_t kl = (uint32_t)std::min<size_t>(key.size(), 256);
        const uint64_t ko = keyBytes_.size();
        keyBytes_.insert(keyBytes_.end(), key.data(), key.data() + kl);
        for (uint32_t i = 0; i < n; ++i) {
            if (slots[i] >= capacity()) return ZRC4_ERR_SLOT_RANGE;
            seedIds_.push_back(slots[i]);
            seedOff_.push_back(ko);
            seedLen_.push_back(kl);
        }
        return ZRC4_OK;
    }

    int crypt(const Rc4Span *spans, uint32_t n) override
    {
        int rc = flushSeeds();
        if (rc != ZRC4_OK) return rc;
        if (n == 0) return ZRC4_OK;
        if (!markOnce(seen_, spans, n)) return ZRC4_ERR_INVALID_ARG;
        return ringCap_ ? cryptReservoir(spans, n) : cryptDirect(spans, n);
    }

    // The engine's broadcast call (rc4_hooks.h).  Direct mode: the grouped,
    // optionally framed, launch over `spans`, then ONE out-of-place grouped
    // launch over `to` on the same stream -- stream order is the keystream
    // order of a slot in both lists -- and one wait.  Two launches rather than
    // the two-round call: at 32 buckets and fewer the one-round calls keep
    // the window kernel (include/zrc4.h).  Reservoir mode: cryptReservoir.
    int cryptBatch(const Rc4Span *spans, uint32_t n, const Rc4ToSpan *to, uint32_t nTo, Rc4Frame *frames,
                   uint32_t bound) override
    {
        if (nTo == 0) return frames ? cryptFrame(spans, n, frames, bound) : crypt(spans, n);
        if (frames && ringCap_) return ZRC4_ERR_INVALID_ARG;
        int rc = flushSeeds();
        if (rc != ZRC4_OK) return rc;
        if (!markOnce(seen_, spans, n) || !markOnce(seenTo_, to, nTo, false)) return ZRC4_ERR_INVALID_ARG;
        toSpans_ += nTo;
        for (uint32_t i = 0; i < nTo; ++i) toBytes_ += to[i].len;
        if (ringCap_) return cryptReservoir(spans, n, to, nTo);

        if (frames && n) {
            if ((rc = launchFramed(spans, n, frames, bound)) != ZRC4_OK) return rc;
        } else {
            es_.clear();
            for (uint32_t i = 0; i < n; ++i)
                if (spans[i].len) es_.push_back({spans[i].slot, spans[i].len, offOf(spans[i].data)});
            for (const Entry &e : es_) tailBytes_ += e.len;
            if (!es_.empty()) {
                buildGrouped(tt_, es_);
                if ((rc = launchGrouped(ctx_, tt_, res_.base, nullptr, sA_)) != ZRC4_OK) return rc;
                ++tailLaunches_;
            }
        }
        eo_.clear();
        for (uint32_t i = 0; i < nTo; ++i) {
            if (!to[i].len) continue;
            Entry e{to[i].slot, to[i].len, offOf(to[i].dst)};
            e.soff = offOf(to[i].src);
            eo_.push_back(e);
            tailBytes_ += e.len;
        }
        if (!eo_.empty()) {
            buildGroupedTo(to_, eo_, toSrc_);
            if ((rc = launchTo(ctx_, to_, toSrc_.p, res_.base, sA_)) != ZRC4_OK) {
                (void)zrc4_sync(ctx_, sA_);      // the in-place launch still runs over the caller's blocks
                return rc;
            }
            ++tailLaunches_;
        }
        if ((rc = zrc4_sync(ctx_, sA_)) != ZRC4_OK) return rc;
        if (frames && n) collectFrames(frames);
        return ZRC4_OK;
    }

    // Device framing rides on the direct mode's launch (the reservoir mode
    // decrypts on the host, so there is no device pass to fuse with).
    bool canFrame() const override { return ringCap_ == 0; }

    int cryptFrame(const Rc4Span *spans, uint32_t n, Rc4Frame *frames, uint32_t bound) override
    {
        if (ringCap_) return ZRC4_ERR_INVALID_ARG;
        int rc = flushSeeds();
        if (rc != ZRC4_OK) return rc;
        if (n == 0) return ZRC4_OK;
        if (!markOnce(seen_, spans, n)) return ZRC4_ERR_INVALID_ARG;
        if ((rc = launchFramed(spans, n, frames, bound)) != ZRC4_OK) return rc;
        if ((rc = zrc4_sync(ctx_, sA_)) != ZRC4_OK) return rc;
        collectFrames(frames);
        return ZRC4_OK;
    }

    std::string stats() const override
    {
        char b[1024];
        std::snprintf(b, sizeof b,
                      "{\"ring_bytes\": %llu, \"tail_bytes\": %llu, \"tail_launches\": %llu, "
                      "\"refill_bytes\": %llu, \"refill_launches\": %llu, \"refill_waits\": %llu, "
                      "\"ring_cap\": %u, \"refill_chunk\": %u, \"device_framed\": %llu, \"xor_threads\": %u, "
                      "\"direct_calls\": %llu, \"direct_bytes\": %llu, \"keystream_launches\": %llu, "
                      "\"to_spans\": %llu, \"to_bytes\": %llu}",
                      (unsigned long long)res_.coveredBytes, tailBytes_, tailLaunches_,
                      (unsigned long long)res_.committedBytes, (unsigned long long)res_.launches,
                      (unsigned long long)res_.waits, ringCap_, refillChunk_, framed_, xor_.threads(), directCalls_,
                      (unsigned long long)directBytes_, (unsigned long long)res_.launches,   // (every refill is a keystream launch)
                      toSpans_, toBytes_);
        return b;
    }

private:
    // Each slot at most once per list (rc4_hooks.h contract): a second span
    // of one slot would consume keystream the first already accounted for.
    // `seen` then holds callStamp_ at the slots of v[0..n).
    // (cryptBatch marks its second list under the first one's stamp: fresh = false)
    template <class S>
    bool markOnce(std::vector<uint32_t> &seen, const S *v, uint32_t n, bool fresh = true)
    {
        if (fresh && ++callStamp_ == 0) {
            std::fill(seen_.begin(), seen_.end(), 0u);
            std::fill(seenTo_.begin(), seenTo_.end(), 0u);
            callStamp_ = 1;
        }
        for (uint32_t i = 0; i < n; ++i) {
            const uint32_t s = v[i].slot;
            if (s >= seen.size() || seen[s] == callStamp_) return false;
            seen[s] = callStamp_;
        }
        return true;
    }

    // The framed grouped launch of cryptFrame on A (no wait), and its results
    // after the wait.
    int launchFramed(const Rc4Span *spans, uint32_t n, const Rc4Frame *frames, uint32_t bound)
    {
        es_.clear();
        for (uint32_t i = 0; i < n; ++i) {
            Entry e{spans[i].slot, spans[i].len, offOf(spans[i].data)};
            e.idx = i;
            e.flen = frames[i].len;
            e.foff = frames[i].len ? offOf(frames[i].block) : 0;
            es_.push_back(e);
            tailBytes_ += spans[i].len;
        }
        buildGrouped(tt_, es_, &ft_);
        zrc4_frame_args fa{ft_.off.p, ft_.len.p, bound, Rc4Frame::kMaxPackets, ft_.npk.p, ft_.used.p,
                           ft_.status.p, ft_.pkt.p};
        const int rc = launchGrouped(ctx_, tt_, res_.base, &fa, sA_);
        if (rc == ZRC4_OK) ++tailLaunches_;
        return rc;
    }
    void collectFrames(Rc4Frame *frames)
    {
        for (uint32_t b = 0; b < tt_.n; ++b) {
            const int64_t i = ft_.idx[b];
            if (i < 0 || !frames[i].len) continue;
            Rc4Frame &f = frames[i];
            f.npk = ft_.npk.p[b];
            f.used = ft_.used.p[b];
            f.status = ft_.status.p[b];
            const uint32_t k = std::min(f.npk, Rc4Frame::kMaxPackets);
            std::memcpy(f.pkt, ft_.pkt.p + (size_t)b * Rc4Frame::kMaxPackets, k * sizeof(uint32_t));
            ++framed_;
        }
    }

    // The grouped layout over out-of-place entries: t.off holds the
    // destinations, soff the sources (padding reads nothing: length 0).
    static void buildGroupedTo(Table &t, std::vector<Entry> &es, PinnedArray<uint64_t> &soff)
    {
        const bool ok = zrc4::buildGrouped(t, es, [&](const Entry *e) {
            soff.reserve(t.n);
            soff.p[t.n - 1] = e ? e->soff : 0;
        });
        if (!ok) throw std::bad_alloc();
    }

    uint64_t offOf(const void *p)
    {
        if (!res_.base) res_.base = static_cast<uint8_t *>(const_cast<void *>(p));
        return (uint64_t)((uintptr_t)p - (uintptr_t)res_.base);
    }

    // One grouped launch on A over `es`, then the wait.
    int runTail(std::vector<Entry> &es)
    {
        if (es.empty()) return ZRC4_OK;
        buildGrouped(tt_, es);
        int rc = launchGrouped(ctx_, tt_, res_.base, nullptr, sA_);
        if (rc != ZRC4_OK) return rc;
        ++tailLaunches_;
        return zrc4_sync(ctx_, sA_);
    }

    int cryptDirect(const Rc4Span *spans, uint32_t n)
    {
        es_.clear();
        for (uint32_t i = 0; i < n; ++i)
            if (spans[i].len) es_.push_back({spans[i].slot, spans[i].len, offOf(spans[i].data)});
        for (const Entry &e : es_) tailBytes_ += e.len;
        return runTail(es_);
    }

    // Adaptive mode (r03).  The reservoir wins while an iteration is small
    // (a host XOR, no GPU round trip on the latency path); with megabytes per
    // iteration the host XOR of every span dominates and one grouped launch
    // over the spans in place (zero-copy pinned blocks) wins: 2048 x 2
    // sessions (~4 MB per call) 134k vs 172k echo/s, 512 x 4 (~1.8 MB) 210k vs
    // 223k, while 512 x 1 (~0.45 MB) runs 228k vs 212k the other way
    // (profiles/r02/frame_loopback_win_v17.jsonl).  So the hooks follow a
    // moving average of the bytes per call: at or above $ZSX_RC4_DIRECT_BYTES
    // (default 1 MiB; 0 = never) they stop refilling -- each slot drains
    // what its ring holds, then its spans go to the device as tails, which
    // is exactly the direct mode's launch -- and below half of it refills
    // resume.  The keystream order is the same either way.
    void updateMode(const Rc4Span *spans, uint32_t n, const Rc4ToSpan *to, uint32_t nTo)
    {
        uint64_t bytes = 0;
        for (uint32_t i = 0; i < n; ++i) bytes += spans[i].len;
        for (uint32_t i = 0; i < nTo; ++i) bytes += to[i].len;
        emaBytes_ = emaBytes_ == 0.0 ? (double)bytes : 0.875 * emaBytes_ + 0.125 * (double)bytes;
        if (directBytes_ && !direct_ && emaBytes_ >= (double)directBytes_) direct_ = true;
        else if (direct_ && emaBytes_ < 0.5 * (double)directBytes_) direct_ = false;
        if (direct_) ++directCalls_;
    }

    // The spans in place, then (cryptBatch) the out-of-place spans `to`, whose
    // keystream follows their slot's in-place span: dst = src ^ ring on the
    // host, and what the ring does not cover is copied to dst and joins the
    // device tail in place.
    int cryptReservoir(const Rc4Span *spans, uint32_t n, const Rc4ToSpan *to = nullptr, uint32_t nTo = 0)
    {
        updateMode(spans, n, to, nTo);
        int rc = pollRefills(false);
        if (rc != ZRC4_OK) return rc;
        if (nTo) {
            // slotAux_[slot], at the slots of `spans` (seen_ holds the stamp):
            // the in-place length here, the slot's tail entry below
            slotAux_.resize(seen_.size());
            for (uint32_t i = 0; i < n; ++i) slotAux_[spans[i].slot] = spans[i].len;
        }
        rc = res_.waitCovered(n + nTo, [&](uint32_t i) {
            if (i < n) return std::pair<uint32_t, uint32_t>(spans[i].slot, spans[i].len);
            const Rc4ToSpan &t = to[i - n];
            const uint64_t need = (uint64_t)t.len + (seen_[t.slot] == callStamp_ ? slotAux_[t.slot] : 0u);
            return std::pair<uint32_t, uint32_t>(t.slot, (uint32_t)std::min<uint64_t>(need, 0xFFFFFFFFu));
        }, zrc4::NoFaults());
        if (rc != ZRC4_OK) return rc;
        // Host XOR with the committed ring bytes (XorPool, after this pass:
        // before any refill is launched, since a refill may write the ring
        // bytes consumed here); collect the uncovered tails.
        es_.clear();
        eo_.clear();
        xj_.clear();
        size_t xjBytes = 0;
        for (uint32_t i = 0; i < n; ++i) {
            const Rc4Span &sp = spans[i];
            if (nTo) slotAux_[sp.slot] = 0;
            if (!sp.len) continue;
            const uint32_t tail = res_.cover(sp.slot, sp.len, [&](uint32_t done, const uint8_t *q, uint32_t k) {
                xj_.push_back({sp.data + done, q, k});
            });
            xjBytes += sp.len - tail;
            if (tail) {
                // the slot's device state is at the end of what the ring covered
                es_.push_back({sp.slot, tail, offOf(sp.data + (sp.len - tail))});
                if (nTo) slotAux_[sp.slot] = (uint32_t)es_.size();
                res_.afterTail(sp.slot, tail);
                tailBytes_ += tail;
            }
            if (!direct_) res_.markHungry(sp.slot);
        }
        for (uint32_t i = 0; i < nTo; ++i) {
            const Rc4ToSpan &t = to[i];
            if (!t.len) continue;
            const uint32_t tail = res_.cover(t.slot, t.len, [&](uint32_t done, const uint8_t *q, uint32_t k) {
                xj_.push_back({t.dst + done, q, k, t.src + done});
            });
            xjBytes += t.len - tail;
            if (tail) {
                uint8_t *d = t.dst + (t.len - tail);
                std::memcpy(d, t.src + (t.len - tail), tail);
                // A slot whose in-place span left a tail too (its ring is then
                // empty: this whole span is tail) may appear once per launch:
                // one entry where the two are adjacent, as a block's staged
                // bytes and the broadcast behind them are; else a second launch.
                const uint32_t k = seen_[t.slot] == callStamp_ ? slotAux_[t.slot] : 0u;
                if (!k) es_.push_back({t.slot, tail, offOf(d)});
                else if (es_[k - 1].off + es_[k - 1].len == offOf(d)) es_[k - 1].len += tail;
                else eo_.push_back({t.slot, tail, offOf(d)});
                res_.afterTail(t.slot, tail);
                tailBytes_ += tail;
            }
            if (!direct_) res_.markHungry(t.slot);
        }
        xor_.run(xj_, xjBytes);
        if (!es_.empty() || !eo_.empty()) {
            if ((rc = drainRefills()) != ZRC4_OK) return rc;     // slot state must be quiet
            if ((rc = runTail(es_)) != ZRC4_OK) return rc;
            if ((rc = runTail(eo_)) != ZRC4_OK) return rc;
        }
        while (!direct_ && !debugNoRefill_ && res_.inflight() < refillDepth_) {
            const uint32_t before = res_.inflight();
            if ((rc = launchRefill()) != ZRC4_OK) return rc;
            if (res_.inflight() == before) break;
        }
        return ZRC4_OK;
    }

    // One background refill (zrc4_reservoir.hpp) as a zrc4_keystream_grouped
    // launch on B, written straight into the pinned host rings: one chunk's
    // chain ~ refillChunk_ x 40 ns.
    int launchRefill()
    {
        const uint32_t before = res_.inflight();
        const int rc = res_.launchRefill([this](const Table &t) { return launchKeystream(ctx_, t, res_.base, sB_); },
                                         [this] { return zrc4_poll_faults(ctx_); });
        if (rc == ZRC4_ERR_OUT_OF_MEMORY) throw std::bad_alloc();   // pinned memory: a ring slab or a table
        if (rc == ZRC4_OK && debugSyncRefill_ && res_.inflight() != before) return drainRefills();
        return rc;
    }

    // Commit every finished refill (wait = every queued one), then report
    // latched device faults of stream B: committed refills have completed, so
    // their faults are in the latch (no stream wait -- a second queued refill
    // keeps running).
    int pollRefills(bool wait)
    {
        const uint64_t before = res_.commits;
        const int rc = wait ? res_.drain(zrc4::NoFaults()) : res_.poll(zrc4::NoFaults());
        if (rc != ZRC4_OK) return rc;
        return res_.commits != before ? zrc4_poll_faults(ctx_) : ZRC4_OK;
    }
    int drainRefills() { return pollRefills(true); }

    // Queued makeSBox calls: one zrc4_ksa ahead of the hook work on A.  In
    // reservoir mode a reseeded slot's unconsumed keystream is dropped: its
    // counters restart, which is what keeps the stale ring bytes from being read.
    int flushSeeds()
    {
        const uint32_t m = (uint32_t)seedIds_.size();
        if (m == 0) return ZRC4_OK;
        int rc;
        if (ringCap_) {
            if ((rc = drainRefills()) != ZRC4_OK) return rc;
            for (uint32_t s : seedIds_) res_.reset(s);
        } else if ((rc = zrc4_sync(ctx_, sA_)) != ZRC4_OK) {
            return rc;
        }
        kIds_.reserve(m);
        kOff_.reserve(m);
        kLen_.reserve(m);
        kBytes_.reserve(std::max<size_t>(keyBytes_.size(), 1));
        std::memcpy(kIds_.p, seedIds_.data(), m * sizeof(uint32_t));
        std::memcpy(kOff_.p, seedOff_.data(), m * sizeof(uint64_t));
        std::memcpy(kLen_.p, seedLen_.data(), m * sizeof(uint32_t));
        if (!keyBytes_.empty()) std::memcpy(kBytes_.p, keyBytes_.data(), keyBytes_.size());
        seedIds_.clear();
        seedOff_.clear();
        seedLen_.clear();
        keyBytes_.clear();
        rc = zrc4_ksa(ctx_, kIds_.p, kBytes_.p, kOff_.p, kLen_.p, m, sA_);
        if (rc != ZRC4_OK) return rc;
        // The key tables are reused by the next flush: wait for this one (seeds
        // happen at connect / accept, not per packet).
        return zrc4_sync(ctx_, sA_);
    }

    void release()
    {
        if (sB_) (void)hipStreamSynchronize(sB_);
        if (sA_) (void)hipStreamSynchronize(sA_);
        res_.release();
        if (sA_) (void)hipStreamDestroy(sA_);
        if (sB_) (void)hipStreamDestroy(sB_);
        if (ctx_) zrc4_destroy(ctx_);
        sA_ = sB_ = nullptr;
        ctx_ = nullptr;
    }

    // 16 KiB per slot per refill (r06; 8 KiB before): a refill launch pays
    // ~6 us of launch, state load and store around its serial chain, and a
    // few-session engine is bound by that chain (config 1: 113.3k -> 117.0k
    // echo/s, scripts/r06_refill_ab.sh)
    static constexpr uint32_t kRefillChunk = 16384;
    const uint32_t refillDepth_ = std::getenv("ZSX_REFILL_DEPTH") ? std::max(1, std::min(2, std::atoi(std::getenv("ZSX_REFILL_DEPTH")))) : zrc4::Reservoir::kMaxDepth;
    const uint64_t directBytes_ = std::getenv("ZSX_RC4_DIRECT_BYTES")
                                     ? std::strtoull(std::getenv("ZSX_RC4_DIRECT_BYTES"), nullptr, 10)
                                     : (1ull << 20);
    double emaBytes_ = 0.0;
    bool direct_ = false;
    unsigned long long directCalls_ = 0;
    const bool debugNoRefill_ = std::getenv("ZSX_RESERVOIR_NO_REFILL") != nullptr;   // test knobs
    const bool debugSyncRefill_ = std::getenv("ZSX_RESERVOIR_SYNC_REFILL") != nullptr;
    const bool ringPoison_ = std::getenv("ZSX_RING_POISON") != nullptr && std::atoi(std::getenv("ZSX_RING_POISON")) != 0;

    zrc4_ctx *ctx_ = nullptr;
    hipStream_t sA_ = nullptr, sB_ = nullptr;
    zrc4::Reservoir res_;                         // (its base is the payload base of every launch here)
    uint32_t ringCap_;
    uint32_t refillChunk_ = 0;
    std::vector<uint32_t> seen_, seenTo_;         // call stamps per slot: the spans, cryptBatch's out-of-place spans
    std::vector<uint32_t> slotAux_;               // per-slot scratch of a reservoir cryptBatch
    uint32_t callStamp_ = 0;
    std::vector<XorJob> xj_;
    XorPool xor_;
    std::vector<Entry> es_, eo_;
    Table tt_;                                    // tail grouped table
    Table to_;                                    // out-of-place grouped table (cryptBatch, direct mode)
    PinnedArray<uint64_t> toSrc_;                 // its source offsets
    FrameTable ft_;                               // framing tables of cryptFrame
    PinnedArray<uint32_t> kIds_, kLen_;
    PinnedArray<uint64_t> kOff_;
    PinnedArray<uint8_t> kBytes_;
    std::vector<uint32_t> seedIds_, seedLen_;
    std::vector<uint64_t> seedOff_;
    std::vector<uint8_t> keyBytes_;
    unsigned long long tailBytes_ = 0, tailLaunches_ = 0, framed_ = 0, toSpans_ = 0, toBytes_ = 0;
};

}  // namespace

std::unique_ptr<Rc4Hooks> makeDeviceRc4Hooks(int device, uint32_t capacity, uint32_t ringBytes)
{
    return std::unique_ptr<Rc4Hooks>(new DeviceRc4Hooks(device, capacity, ringBytes));
}

}  // namespace zsummerx_amd
