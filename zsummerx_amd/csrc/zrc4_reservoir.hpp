// zrc4_reservoir.hpp -- the keystream-reservoir core: one host-side
// implementation behind both owners, the C-ABI reservoir (zrc4_ks.inc, compiled
// by hipcc inside zrc4.hip) and the session engine's hooks
// (engine/rc4_hooks_device.cpp, compiled by g++).  Standard library and the
// host HIP runtime API only: no kernels, no launch of its own.
//
// RC4's keystream does not depend on the data, so per slot the device
// generates keystream AHEAD into a ring of pinned host memory; a consumer XORs
// its bytes with committed ring bytes on the host and goes to the device only
// for what the ring does not cover (a "tail").  Refills are write-only grouped
// launches (the owner's callable) on a background stream, at most `depth`
// queued, each committed once its event has completed.
//
// Invariants (per slot: gen = end of committed keystream, use = bytes
// consumed, pend = end of queued refills; the device state sits at pend):
//   * use <= gen <= pend and pend - use <= ring; pend > gen only while a
//     refill is queued;
//   * the host reads only ring bytes in [use, gen) (cover); a refill writes
//     only [pend, pend + chunk), which the ring size keeps clear of them.  The
//     levels alone say which ring bytes hold keystream: consumed bytes, a
//     reset slot's dropped ones and a fresh slab's contents stay as they are
//     until a refill overwrites them, and are never read (the fill byte shows
//     it: a byte read outside the levels cannot pass for zero);
//   * kernels that touch slot state (seed, tail crypt, state copy, refill)
//     never run beside each other: a grouped kernel stores its whole 64 KiB
//     group image, so the owner drain()s before a seed, a tail or a copy, and
//     then resets the slot or sets gen = pend = use (afterTail);
//   * refills run in stream order and commit in that order;
//   * a launch that fails leaves every level where it was (rings are
//     allocated before any level moves, pend is rolled back when the launch
//     is refused): pend > gen with nothing queued would make waitCovered wait
//     for bytes that never come.
// One thread at a time per reservoir (the owners see to it).
//
// Fault polls (zrc4_poll_faults) stay with the owners, as a callable: commit
// paths call it after the refill has completed and BEFORE its bytes are
// committed (the C-ABI reservoir's order; the engine passes NoFaults there
// and polls once after a batch of commits), launchRefill after the commit of
// a refill whose event could not be recorded.
#ifndef ZRC4_RESERVOIR_HPP
#define ZRC4_RESERVOIR_HPP

#include <hip/hip_runtime_api.h>

#include <algorithm>
#include <cstdint>
#include <cstring>
#include <utility>
#include <vector>

#include "zrc4.h"

namespace zrc4 {
// (libzrc4.so exports the C ABI only, and calls into the core bind directly)
#define ZRC4_CORE_LOCAL __attribute__((visibility("hidden")))

// Growable pinned array; reserve() keeps the entries already written.
template <class T>
struct ZRC4_CORE_LOCAL Pinned {
    T *p = nullptr;
    size_t cap = 0;
    Pinned() = default;
    Pinned(const Pinned &) = delete;
    Pinned &operator=(const Pinned &) = delete;
    ~Pinned()
    {
        if (p) (void)hipHostFree(p);
    }
    bool reserve(size_t n, unsigned flags)
    {
        if (n <= cap) return true;
        size_t c = cap ? cap : 1024;
        while (c < n) c *= 2;
        T *q = nullptr;
        if (hipHostMalloc(reinterpret_cast<void **>(&q), c * sizeof(T), flags) != hipSuccess) return false;
        if (p) {
            std::memcpy(q, p, cap * sizeof(T));
            (void)hipHostFree(p);
        }
        p = q;
        cap = c;
        return true;
    }
};

// One grouped batch (zrc4_crypt_grouped contract) in pinned tables.
struct ZRC4_CORE_LOCAL GroupedTable {
    Pinned<uint32_t> ids, len;
    Pinned<uint64_t> off;
    std::vector<uint32_t> groups;   // each bucket's group, for the declared launches
    uint32_t n = 0;
    unsigned flags = hipHostMallocCoherent;
    bool push(uint32_t id, uint64_t o, uint32_t l)
    {
        if ((n == ids.cap || n == off.cap || n == len.cap) &&
            !(ids.reserve(n + 1, flags) && off.reserve(n + 1, flags) && len.reserve(n + 1, flags)))
            return false;
        ids.p[n] = id;
        off.p[n] = o;
        len.p[n] = l;
        ++n;
        return true;
    }
};

// The grouped layout: entries (anything with slot / off / len) sorted by slot,
// a new 256-entry bucket at every group change (a group holds at most 256
// distinct slots, so one bucket per group), earlier buckets padded with idle
// entries, the last one not.  pushed(e) runs after every table entry, e ==
// nullptr for padding (the engine's framing tables ride on it).  false: out of
// pinned memory.
template <class E, class F>
bool buildGrouped(GroupedTable &t, std::vector<E> &es, F &&pushed)
{
    std::sort(es.begin(), es.end(), [](const E &a, const E &b) { return a.slot < b.slot; });
    t.n = 0;
    t.groups.clear();
    uint32_t cur = ZRC4_IDLE_SLOT;
    for (const E &e : es) {
        const uint32_t g = e.slot / ZRC4_GROUP_SLOTS;
        if (g != cur) {
            while (t.n % ZRC4_GROUP_SLOTS) {
                if (!t.push(ZRC4_IDLE_SLOT, 0, 0)) return false;
                pushed(static_cast<const E *>(nullptr));
            }
            cur = g;
            t.groups.push_back(g);
        }
        if (!t.push(e.slot, e.off, e.len)) return false;
        pushed(&e);
    }
    return true;
}
template <class E>
bool buildGrouped(GroupedTable &t, std::vector<E> &es)
{
    return buildGrouped(t, es, [](const E *) {});
}

struct NoFaults {
    int operator()() const { return ZRC4_OK; }
};

class ZRC4_CORE_LOCAL Reservoir {
public:
    struct Level {
        uint64_t gen = 0;    // keystream bytes generated and committed (absolute stream position)
        uint64_t use = 0;    // keystream bytes consumed
        uint64_t pend = 0;   // end of the last queued refill (== gen when none is queued)
    };
    struct Entry {
        uint32_t slot, len;
        uint64_t off;
    };
    // One queued refill: its table, its completion event and the (slot, end
    // position) pairs it commits.
    struct Refill {
        GroupedTable t;
        hipEvent_t ev = nullptr;
        std::vector<std::pair<uint32_t, uint64_t>> ends;
    };
    static constexpr uint32_t kMaxDepth = 2;

    // Offsets in refill tables are relative to base: the owner's, when it has
    // set one (the engine: its first SessionBlock slab), else the first ring slab.
    uint8_t *base = nullptr;
    // ring bytes handed out, refill bytes queued / committed, refills launched /
    // committed, waits for a queued refill
    uint64_t coveredBytes = 0, queuedBytes = 0, committedBytes = 0, launches = 0, commits = 0, waits = 0;

    ~Reservoir() { release(); }

    // ring bytes per slot (0: no reservoir -- every span is a tail), chunk
    // bytes per slot per refill, depth refills queued at most, on `stream`;
    // slabs and tables from hipHostMalloc(flags), fresh slabs filled with
    // `fill` unless negative.
    int init(uint32_t slots, uint32_t ring, uint32_t chunk, uint32_t depth, hipStream_t stream, unsigned flags,
             int fill = -1)
    {
        ring_ = ring;
        chunk_ = chunk;
        depth_ = std::max(1u, std::min(depth, kMaxDepth));
        stream_ = stream;
        flags_ = flags;
        fill_ = fill;
        lv_.assign(slots, Level());
        slab_.assign((slots + ZRC4_GROUP_SLOTS - 1) / ZRC4_GROUP_SLOTS, nullptr);
        mark_.assign(slots, 0);
        for (Refill &r : rf_) {
            r.t.flags = flags;
            if (hipEventCreateWithFlags(&r.ev, hipEventDisableTiming) != hipSuccess) return ZRC4_ERR_HIP;
        }
        return ZRC4_OK;
    }
    // (the owner has waited for the stream)
    void release()
    {
        for (Refill &r : rf_) {
            if (r.ev) (void)hipEventDestroy(r.ev);
            r.ev = nullptr;
        }
        for (uint8_t *&s : slab_) {
            if (s) (void)hipHostFree(s);
            s = nullptr;
        }
    }

    uint32_t ring() const { return ring_; }
    uint32_t inflight() const { return inflight_; }
    const Level &level(uint32_t s) const { return lv_[s]; }
    const std::vector<uint32_t> &hungry() const { return hungry_; }
    bool marked(uint32_t s) const { return mark_[s] != 0; }
    const Refill &refill(uint32_t i) const { return rf_[i]; }

    // The ring of slot s: one slab of 256 rings per group, allocated on first
    // use and left as it comes.  nullptr: out of pinned memory.
    uint8_t *ringOf(uint32_t s)
    {
        uint8_t *&sl = slab_[s / ZRC4_GROUP_SLOTS];
        if (!sl) {
            const size_t bytes = (size_t)ZRC4_GROUP_SLOTS * ring_;
            void *p = nullptr;
            if (hipHostMalloc(&p, bytes, flags_) != hipSuccess) return nullptr;
            if (fill_ >= 0) std::memset(p, fill_, bytes);
            sl = static_cast<uint8_t *>(p);
            if (!base) base = sl;
        }
        return sl + (size_t)(s % ZRC4_GROUP_SLOTS) * ring_;
    }

    // A reseeded slot, or one whose ring the owner filled with `buffered` bytes
    // from its start (the levels guard the ring bytes: the rest is never read).
    void reset(uint32_t s, uint64_t buffered = 0) { lv_[s] = Level{buffered, 0, buffered}; }

    // A slot consumed from is refilled by the next launchRefill.
    void markHungry(uint32_t s)
    {
        if (ring_ && !mark_[s]) {
            mark_[s] = 1;
            hungry_.push_back(s);
        }
    }

    // The committed keystream of the next `len` bytes of slot s, consumed:
    // piece(done, ring bytes, count) for at most two pieces (ring wrap), done
    // = bytes of the span before the piece.  Returns the uncovered tail length.
    template <class Piece>
    uint32_t cover(uint32_t s, uint32_t len, Piece &&piece)
    {
        Level &L = lv_[s];
        const uint32_t have = (uint32_t)std::min<uint64_t>(L.gen - L.use, len);
        if (have) {
            const uint8_t *r = ringAt(s);          // exists: a refill was committed into it
            for (uint32_t done = 0; done < have;) {
                const uint32_t at = (uint32_t)((L.use + done) % ring_);
                const uint32_t m = std::min(have - done, ring_ - at);
                piece(done, r + at, m);
                done += m;
            }
            L.use += have;
            coveredBytes += have;
        }
        return len - have;
    }

    // The device crypted a tail of `len` bytes of slot s with nothing queued
    // for it: its state sits at the new use, and the ring holds nothing.
    void afterTail(uint32_t s, uint32_t len)
    {
        Level &L = lv_[s];
        L.use += len;
        L.gen = L.pend = L.use;
    }

    // Commit the oldest queued refill if it has finished (wait: block until it
    // has); `ready` says whether one was committed.
    template <class Faults>
    int commitOldest(bool wait, Faults &&faults, bool *ready = nullptr)
    {
        if (ready) *ready = false;
        if (!inflight_) return ZRC4_OK;
        Refill &R = rf_[head_];
        if (wait) {
            if (hipEventSynchronize(R.ev) != hipSuccess) return ZRC4_ERR_HIP;
        } else {
            const hipError_t q = hipEventQuery(R.ev);
            if (q == hipErrorNotReady) return ZRC4_OK;
            if (q != hipSuccess) return ZRC4_ERR_HIP;
        }
        const int rc = faults();
        if (rc != ZRC4_OK) return rc;
        commit(R);
        head_ = (head_ + 1) % kMaxDepth;
        --inflight_;
        if (ready) *ready = true;
        return ZRC4_OK;
    }
    // Commit every refill that has finished.
    template <class Faults>
    int poll(Faults &&faults)
    {
        for (bool ready = true; ready && inflight_;) {
            const int rc = commitOldest(false, faults, &ready);
            if (rc != ZRC4_OK) return rc;
        }
        return ZRC4_OK;
    }
    // Wait for and commit every queued refill.
    template <class Faults>
    int drain(Faults &&faults)
    {
        while (inflight_) {
            const int rc = commitOldest(true, faults);
            if (rc != ZRC4_OK) return rc;
        }
        return ZRC4_OK;
    }
    // A span short of committed keystream while refills are queued for its
    // slot: wait for them in order until every span is covered or none is left
    // (their bytes are the ones it needs, and a tail crypt may not run beside
    // them).  span(i) -> {slot, len} for i < n.
    template <class Span, class Faults>
    int waitCovered(uint32_t n, Span &&span, Faults &&faults)
    {
        while (inflight_) {
            bool wait = false;
            for (uint32_t i = 0; i < n && !wait; ++i) {
                const std::pair<uint32_t, uint32_t> sp = span(i);
                const Level &L = lv_[sp.first];
                wait = L.gen - L.use < sp.second && L.pend > L.gen;
            }
            if (!wait) break;                    // (nothing queued: the span goes to the tail path)
            ++waits;
            const int rc = commitOldest(true, faults);
            if (rc != ZRC4_OK) return rc;
        }
        return ZRC4_OK;
    }

    // One write-only grouped launch, launch(table) -> ZRC4 code, into the
    // rings' next free bytes of every hungry slot.  Whole chunks only: a launch
    // lasts as long as its longest piece (one lane per slot), so every slot it
    // carries gets a full chunk (or the piece up to the ring end); a slot
    // without room for one leaves the hungry list until it is consumed from
    // again.  Up to `depth` refills are queued back to back, so keystream
    // generation does not pause between launches (stream order keeps each
    // slot's pieces sequential).
    template <class Launch, class Faults>
    int launchRefill(Launch &&launch, Faults &&faults)
    {
        if (!ring_ || inflight_ >= depth_ || hungry_.empty()) return ZRC4_OK;
        Refill &R = rf_[(head_ + inflight_) % kMaxDepth];
        keep_.clear();                            // (one pass over the whole list: the slots with room are few)
        for (uint32_t s : hungry_) {
            if (room(lv_[s])) keep_.push_back(s);
            else mark_[s] = 0;
        }
        hungry_.swap(keep_);
        for (uint32_t s : hungry_)                // rings first: no level moves if one cannot be had
            if (!ringOf(s)) return ZRC4_ERR_OUT_OF_MEMORY;
        es_.clear();
        R.ends.clear();
        uint64_t bytes = 0;
        for (uint32_t s : hungry_) {
            Level &L = lv_[s];
            const uint32_t at = (uint32_t)(L.pend % ring_);
            const uint32_t amt = std::min(ring_ - at, chunk_);
            es_.push_back({s, amt, (uint64_t)((uintptr_t)(ringAt(s) + at) - (uintptr_t)base)});
            L.pend += amt;
            R.ends.push_back({s, L.pend});
            bytes += amt;
        }
        if (es_.empty()) return ZRC4_OK;
        const int rc = buildGrouped(R.t, es_) ? launch(static_cast<const GroupedTable &>(R.t)) : ZRC4_ERR_OUT_OF_MEMORY;
        if (rc != ZRC4_OK) {                      // nothing queued: the levels go back
            for (const Entry &e : es_) lv_[e.slot].pend -= e.len;
            R.ends.clear();
            return rc;
        }
        ++launches;
        queuedBytes += bytes;
        if (hipEventRecord(R.ev, stream_) != hipSuccess) {
            // queued but untrackable: wait for the stream and commit it now
            if (hipStreamSynchronize(stream_) != hipSuccess) return ZRC4_ERR_HIP;
            commit(R);
            return faults();
        }
        ++inflight_;
        return ZRC4_OK;
    }

private:
    uint8_t *ringAt(uint32_t s) const { return slab_[s / ZRC4_GROUP_SLOTS] + (size_t)(s % ZRC4_GROUP_SLOTS) * ring_; }
    bool room(const Level &L) const { return ring_ - (L.pend - L.use) >= chunk_; }
    void commit(Refill &R)
    {
        for (const auto &e : R.ends) {
            Level &L = lv_[e.first];
            if (e.second > L.gen) {
                committedBytes += e.second - L.gen;
                L.gen = e.second;
            }
        }
        R.ends.clear();
        ++commits;
    }

    uint32_t ring_ = 0, chunk_ = 0, depth_ = kMaxDepth;
    hipStream_t stream_ = nullptr;
    unsigned flags_ = hipHostMallocCoherent;
    int fill_ = -1;
    std::vector<Level> lv_;
    std::vector<uint8_t *> slab_;
    std::vector<uint8_t> mark_;
    std::vector<uint32_t> hungry_, keep_;
    Refill rf_[kMaxDepth];
    uint32_t head_ = 0, inflight_ = 0;
    std::vector<Entry> es_;
};

}  // namespace zrc4

#endif
