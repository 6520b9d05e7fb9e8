// zrc4_ks.inc -- keystream reservoirs over a context (include/zrc4.h,
// zrc4_ks_*), included by zrc4.hip.
//
// The per-call RC4Encryption::encryption (rc4_encryption.h:74-93) of the C++
// mirror used to be one launch and one wait per call: ~15 us of round trip
// plus the serial chain of the call's bytes.  RC4's keystream does not depend
// on the data, so a reservoir keeps, per slot, keystream the device generated
// AHEAD into a ring of pinned host memory; a call XORs the caller's bytes with
// committed ring bytes on the host and goes to the device only for what the
// ring does not cover (a "tail", e.g. a slot's first call after makeSBox).
// Refills run in the background on their own stream: one write-only grouped
// launch (launch_crypt with io = kIoKs, the path of zrc4_keystream_grouped) that
// STORES the next keystream bytes of every slot used since the last refill
// into its ring, whatever the ring held -- it is never read by the device and
// never zeroed by the host -- at most kDepth queued, committed when their
// event has completed.
// The RC4 state never leaves the device and keystream bytes are consumed in
// order, so every output byte is the reference's.
//
// Invariants (per slot: gen = end of committed keystream, use = bytes
// consumed, pend = end of queued refills; the device state sits at pend):
//   * the host reads only ring bytes in [use, gen); refills write only
//     [pend, pend + chunk), which the ring size keeps clear of [use, gen).
//     The levels alone say which ring bytes hold keystream: consumed bytes
//     (and a reseeded slot's dropped ones) stay in the ring, stale, until a
//     later refill overwrites them;
//   * a tail crypt, a reseed or a state copy first drains every queued refill
//     (a grouped kernel stores whole 64 KiB group images), then gen = pend =
//     use for the slots it touches;
//   * every entry point takes the reservoir's mutex: one thread at a time per
//     reservoir (and the context's staging buffers with it).
// Same design as the session engine's reservoir hooks
// (zsummerx_amd/engine/rc4_hooks_device.cpp), at the C-ABI so the mirror and
// any other per-call user can have it.

#include <mutex>

namespace {

template <class T>
struct PinnedVec {
    T *p = nullptr;
    size_t cap = 0;
    bool reserve(size_t n)
    {
        if (n <= cap) return true;
        size_t c = cap ? cap : 1024;
        while (c < n) c *= 2;
        T *q = nullptr;
        if (hipHostMalloc(reinterpret_cast<void **>(&q), c * sizeof(T), hipHostMallocCoherent) != hipSuccess)
            return false;
        if (p) (void)hipHostFree(p);
        p = q;
        cap = c;
        return true;
    }
    void release()
    {
        if (p) (void)hipHostFree(p);
        p = nullptr;
        cap = 0;
    }
};

struct KsLevel {
    uint64_t gen = 0, use = 0, pend = 0;
    bool lost = false;    // a failed tail crypt: position unknown until reseeded or copied into
};

struct KsEntry {
    uint32_t slot, len;
    uint64_t off;
};

// A grouped batch (zrc4_crypt_grouped contract) in pinned tables.
struct KsTable {
    PinnedVec<uint32_t> ids, len;
    PinnedVec<uint64_t> off;
    std::vector<uint32_t> groups;   // each bucket's group (declared to the launch)
    uint32_t n = 0;
    bool build(std::vector<KsEntry> &es)
    {
        std::sort(es.begin(), es.end(), [](const KsEntry &a, const KsEntry &b) { return a.slot < b.slot; });
        groups.clear();
        for (size_t i = 0; i < es.size(); ++i)
            if (!i || (es[i].slot >> 8) != (es[i - 1].slot >> 8)) groups.push_back(es[i].slot >> 8);
        const uint32_t buckets = (uint32_t)groups.size();
        n = buckets * zrc4::kGroup;
        if (!ids.reserve(n) || !len.reserve(n) || !off.reserve(n)) return false;
        for (uint32_t e = 0; e < n; ++e) {
            ids.p[e] = ZRC4_IDLE_SLOT;
            len.p[e] = 0;
            off.p[e] = 0;
        }
        uint32_t b = 0, pos = 0;
        for (size_t i = 0; i < es.size(); ++i) {
            if (i && (es[i].slot >> 8) != (es[i - 1].slot >> 8)) {
                ++b;
                pos = 0;
            }
            const uint32_t e = b * zrc4::kGroup + pos++;
            ids.p[e] = es[i].slot;
            len.p[e] = es[i].len;
            off.p[e] = es[i].off;
        }
        return true;
    }
    void release()
    {
        ids.release();
        len.release();
        off.release();
    }
};

struct KsRefill {
    KsTable t;
    hipEvent_t ev = nullptr;
    std::vector<std::pair<uint32_t, uint64_t>> ends;
};

}  // namespace

struct zrc4_ks {
    static constexpr uint32_t kDepth = 2;
    zrc4_ctx *c = nullptr;
    uint32_t ring = 0, chunk = 0;
    hipStream_t sB = nullptr;
    std::mutex mu;
    std::vector<KsLevel> lv;
    std::vector<uint8_t *> slab;          // per 256-slot group: 256 rings, allocated on first use
    uint8_t *base = nullptr;              // offsets in refill tables are relative to the first slab
    std::vector<uint8_t> hungryMark;
    std::vector<uint32_t> hungry;
    KsRefill rf[kDepth];
    uint32_t head = 0, inflight = 0;
    std::vector<KsEntry> es;
    std::vector<uint8_t> tailBuf;
    std::vector<uint32_t> tailIds, tailLen;
    std::vector<uint64_t> tailOff;
    std::vector<uint8_t *> tailDst;
    uint64_t st[6] = {0, 0, 0, 0, 0, 0};  // ring bytes, tail bytes, tail launches, refill bytes, launches, waits
    uint64_t refillFailures = 0;          // refills that could not be queued (retried by the next call)
    // Test hook, in ZRC4_TEST_HOOKS builds only (libzrc4_testhooks.so):
    // $ZRC4_KS_FAIL_TAIL_AFTER = n makes the n-th tail crypt of this reservoir
    // fail before launching (tests/test_gpu_parity.py: a failed call loses
    // its slots' positions -> ZRC4_ERR_STATE until reseeded).
    uint64_t failTailsAfter = 0, tailCalls = 0;

    uint8_t *ringOf(uint32_t s)
    {
        uint8_t *&sl = slab[s / zrc4::kGroup];
        if (!sl) {
            void *p = nullptr;
            const size_t bytes = (size_t)zrc4::kGroup * ring;
            if (hipHostMalloc(&p, bytes, hipHostMallocCoherent) != hipSuccess) return nullptr;
            sl = static_cast<uint8_t *>(p);
            if (!base) base = sl;
        }
        return sl + (size_t)(s % zrc4::kGroup) * ring;
    }

    int commitOldest(bool wait)
    {
        if (!inflight) return ZRC4_OK;
        KsRefill &R = rf[head];
        if (wait) {
            ZRC4_TRY(hipEventSynchronize(R.ev));
        } else {
            const hipError_t q = hipEventQuery(R.ev);
            if (q == hipErrorNotReady) return ZRC4_OK;
            if (q != hipSuccess) return ZRC4_ERR_HIP;
        }
        const int rc = zrc4_poll_faults(c);
        if (rc != ZRC4_OK) return rc;
        for (const auto &e : R.ends) lv[e.first].gen = e.second;
        head = (head + 1) % kDepth;
        --inflight;
        return ZRC4_OK;
    }
    int poll()
    {
        while (inflight) {
            const uint32_t before = inflight;
            const int rc = commitOldest(false);
            if (rc != ZRC4_OK) return rc;
            if (inflight == before) break;
        }
        return ZRC4_OK;
    }
    int drain()
    {
        while (inflight) {
            const int rc = commitOldest(true);
            if (rc != ZRC4_OK) return rc;
        }
        return ZRC4_OK;
    }

    // One write-only grouped launch into the rings' next free bytes of every
    // hungry slot (whole chunks only: a launch lasts as long as its longest piece).
    int launchRefill()
    {
        if (!ring || inflight >= kDepth || hungry.empty()) return ZRC4_OK;
        KsRefill &R = rf[(head + inflight) % kDepth];
        es.clear();
        R.ends.clear();
        for (uint32_t s : hungry)                 // rings first: no level moves if one cannot be had
            if (!ringOf(s)) return ZRC4_ERR_OUT_OF_MEMORY;
        std::vector<uint32_t> keep;
        for (uint32_t s : hungry) {
            KsLevel &L = lv[s];
            if (ring - (L.pend - L.use) < chunk) {
                hungryMark[s] = 0;
                continue;
            }
            uint8_t *r = ringOf(s);
            const uint32_t at = (uint32_t)(L.pend % ring);
            const uint32_t amt = std::min(ring - at, chunk);
            es.push_back({s, amt, (uint64_t)((uintptr_t)(r + at) - (uintptr_t)base)});
            L.pend += amt;
            R.ends.push_back({s, L.pend});
            keep.push_back(s);
            st[3] += amt;
        }
        hungry.swap(keep);
        if (es.empty()) return ZRC4_OK;
        // (the groups built here are declared to the launch; trusted: no
        // up-front check above 256 buckets, where they are not used)
        int rc = R.t.build(es) ? (set_device(c) ? ZRC4_ERR_HIP : ZRC4_OK) : ZRC4_ERR_OUT_OF_MEMORY;
        if (rc == ZRC4_OK) {
            CryptCall k = crypt_call(zrc4::kGrouped, R.t.ids.p, 0, base, R.t.off.p, R.t.len.p, R.t.n);
            k.decl = R.t.groups.data();
            k.trusted = true;
            k.io = zrc4::kIoKs;
            rc = launch_crypt(c, k, sB);
        }
        if (rc != ZRC4_OK) {                      // nothing queued: the levels go back
            for (const KsEntry &e : es) lv[e.slot].pend -= e.len;
            return rc;
        }
        ++st[4];
        if (hipEventRecord(R.ev, sB) != hipSuccess) {
            // queued but untrackable: wait for stream B and commit it now
            ZRC4_TRY(hipStreamSynchronize(sB));
            for (const auto &e : R.ends)
                if (e.second > lv[e.first].gen) lv[e.first].gen = e.second;
            R.ends.clear();
            return zrc4_poll_faults(c);
        }
        ++inflight;
        return ZRC4_OK;
    }

    // The device crypts the uncovered tails of a call (host spans), as one
    // zrc4_crypt_host batch (grouped when several).
    int runTails()
    {
        if (tailIds.empty()) return ZRC4_OK;
        int rc = drain();
        if (rc != ZRC4_OK) return rc;
        if (failTailsAfter && ++tailCalls == failTailsAfter) return ZRC4_ERR_HIP;   // fault injection (tests)
        rc = zrc4_crypt_host(c, tailIds.data(), tailBuf.data(), tailBuf.size(), tailOff.data(), tailLen.data(),
                             (uint32_t)tailIds.size());
        if (rc != ZRC4_OK) return rc;
        for (size_t i = 0; i < tailIds.size(); ++i) memcpy(tailDst[i], tailBuf.data() + tailOff[i], tailLen[i]);
        ++st[2];
        return ZRC4_OK;
    }

    // (the levels guard the ring bytes: what the ring still holds is never read)
    void resetRing(uint32_t s) { lv[s] = KsLevel{}; }
};

extern "C" {

int zrc4_ks_create(zrc4_ctx *c, uint32_t ring_bytes, zrc4_ks **out)
{
    if (!c || !out) return ZRC4_ERR_INVALID_ARG;
    *out = nullptr;
    int rc = set_device(c);
    if (rc) return rc;
    zrc4_ks *k = new (std::nothrow) zrc4_ks;
    if (!k) return ZRC4_ERR_OUT_OF_MEMORY;
    k->c = c;
    k->ring = ring_bytes;
#if defined(ZRC4_TEST_HOOKS) && ZRC4_TEST_HOOKS
    if (const char *f = getenv("ZRC4_KS_FAIL_TAIL_AFTER")) {
        k->failTailsAfter = strtoull(f, nullptr, 10);
        fprintf(stderr, "zrc4: test hook active: tail crypt %llu of this reservoir will fail\n",
                (unsigned long long)k->failTailsAfter);
    }
#endif
    // A quarter ring per refill: two refills stay queued while the consumer
    // keeps up (with half-ring chunks a slot had room for the next refill only
    // once the previous one was consumed, and the device idled between them).
    k->chunk = ring_bytes ? std::max<uint32_t>(64u, ring_bytes / 4u) : 0u;
    k->lv.resize(c->capacity);
    k->slab.assign(c->capacity / zrc4::kGroup, nullptr);
    k->hungryMark.assign(c->capacity, 0);
    bool ok = hipStreamCreateWithFlags(&k->sB, hipStreamNonBlocking) == hipSuccess;
    for (KsRefill &r : k->rf) ok = ok && hipEventCreateWithFlags(&r.ev, hipEventDisableTiming) == hipSuccess;
    if (!ok) {
        zrc4_ks_destroy(k);
        return ZRC4_ERR_HIP;
    }
    *out = k;
    return ZRC4_OK;
}

int zrc4_ks_destroy(zrc4_ks *k)
{
    if (!k) return ZRC4_ERR_INVALID_ARG;
    {
        std::lock_guard<std::mutex> g(k->mu);
        (void)k->drain();
        if (k->sB) (void)hipStreamSynchronize(k->sB);
        for (KsRefill &r : k->rf) {
            if (r.ev) (void)hipEventDestroy(r.ev);
            r.t.release();
        }
        if (k->sB) (void)hipStreamDestroy(k->sB);
        for (uint8_t *s : k->slab)
            if (s) (void)hipHostFree(s);
    }
    delete k;
    return ZRC4_OK;
}

int zrc4_ks_crypt(zrc4_ks *k, const uint32_t *ids, uint8_t *const *data, const uint32_t *len, uint32_t n)
{
    if (!k || (n && (!ids || !data || !len))) return ZRC4_ERR_INVALID_ARG;
    std::lock_guard<std::mutex> g(k->mu);
    for (uint32_t i = 0; i < n; ++i) {
        if (ids[i] >= k->c->capacity) return ZRC4_ERR_SLOT_RANGE;
        if (len[i] && !data[i]) return ZRC4_ERR_INVALID_ARG;
        const KsLevel &L = k->lv[ids[i]];
        if (L.lost || L.gen < L.use) return ZRC4_ERR_STATE;
    }
    // a slot once per call (the keystream of a second span would be the first's)
    if (n > 1) {
        std::vector<uint32_t> v(ids, ids + n);
        std::sort(v.begin(), v.end());
        for (uint32_t i = 1; i < n; ++i)
            if (v[i] == v[i - 1]) return ZRC4_ERR_INVALID_ARG;
    }
    int rc = set_device(k->c);
    if (rc) return rc;
    if ((rc = k->poll()) != ZRC4_OK) return rc;
    // A slot short of committed keystream while refills are queued: wait for
    // them in order until it is covered or none is left.
    for (;;) {
        bool wait = false;
        for (uint32_t i = 0; i < n && !wait; ++i) {
            const KsLevel &L = k->lv[ids[i]];
            if (L.gen - L.use < len[i] && L.pend > L.gen) wait = true;
        }
        if (!wait || !k->inflight) break;
        ++k->st[5];
        if ((rc = k->commitOldest(true)) != ZRC4_OK) return rc;
    }
    k->tailIds.clear();
    k->tailLen.clear();
    k->tailOff.clear();
    k->tailDst.clear();
    k->tailBuf.clear();
    for (uint32_t i = 0; i < n; ++i) {
        const uint32_t s = ids[i];
        if (!len[i]) continue;
        KsLevel &L = k->lv[s];
        const uint32_t have = (uint32_t)std::min<uint64_t>(L.gen - L.use, len[i]);
        if (have) {
            uint8_t *r = k->ringOf(s);
            uint32_t done = 0;
            while (done < have) {
                const uint32_t at = (uint32_t)((L.use + done) % k->ring);
                const uint32_t m = std::min(have - done, k->ring - at);
                uint8_t *d = data[i] + done, *q = r + at;
                for (uint32_t b = 0; b < m; ++b) d[b] ^= q[b];
                done += m;
            }
            L.use += have;
            k->st[0] += have;
        }
        if (have < len[i]) {
            const uint32_t t = len[i] - have;
            k->tailIds.push_back(s);
            k->tailLen.push_back(t);
            k->tailOff.push_back(k->tailBuf.size());
            k->tailDst.push_back(data[i] + have);
            k->tailBuf.insert(k->tailBuf.end(), data[i] + have, data[i] + len[i]);
            k->st[1] += t;                       // use moves only once the tail crypt succeeded
        }
        if (k->ring && !k->hungryMark[s]) {
            k->hungryMark[s] = 1;
            k->hungry.push_back(s);
        }
    }
    if (!k->tailIds.empty()) {
        if ((rc = k->runTails()) != ZRC4_OK) {
            // The device may or may not have advanced the tail slots, and the
            // ring-covered spans of this call are already crypted: the call
            // fails as a whole, so every slot of it is lost (ZRC4_ERR_STATE
            // on later calls) until reseeded or copied into -- a caller
            // cannot retry part of a batch it cannot see.
            for (uint32_t i = 0; i < n; ++i)
                if (len[i]) k->lv[ids[i]].lost = true;
            return rc;
        }
        for (size_t t = 0; t < k->tailIds.size(); ++t) {
            KsLevel &L = k->lv[k->tailIds[t]];
            L.use += k->tailLen[t];
            L.gen = L.pend = L.use;
        }
    }
    // Background refills are best-effort for this call: its bytes are already
    // crypted, so a refill that cannot be queued now (pinned-memory or launch
    // failure) is retried by the next call, which crypts on the device what
    // the rings then lack.  Hard errors are reserved for the tail path.
    while (k->inflight < zrc4_ks::kDepth) {
        const uint32_t before = k->inflight;
        if (k->launchRefill() != ZRC4_OK) {
            ++k->refillFailures;
            break;
        }
        if (k->inflight == before) break;
    }
    return ZRC4_OK;
}

int zrc4_ks_make_sbox(zrc4_ks *k, uint32_t id, const uint8_t *key, size_t keylen)
{
    if (!k) return ZRC4_ERR_INVALID_ARG;
    std::lock_guard<std::mutex> g(k->mu);
    if (id >= k->c->capacity) return ZRC4_ERR_SLOT_RANGE;
    int rc = set_device(k->c);
    if (rc) return rc;
    if ((rc = k->drain()) != ZRC4_OK) return rc;        // no refill may touch the slot's group now
    if ((rc = zrc4_make_sbox(k->c, id, key, keylen)) != ZRC4_OK) return rc;
    k->resetRing(id);
    return ZRC4_OK;
}

int zrc4_ks_copy(zrc4_ks *dk, uint32_t dst, zrc4_ks *sk, uint32_t src)
{
    if (!dk || !sk) return ZRC4_ERR_INVALID_ARG;
    if (dk == sk && dst == src) return ZRC4_OK;
    // both reservoirs locked, in address order
    std::unique_lock<std::mutex> l1(dk < sk ? dk->mu : sk->mu, std::defer_lock);
    std::unique_lock<std::mutex> l2(dk < sk ? sk->mu : dk->mu, std::defer_lock);
    l1.lock();
    if (dk != sk) l2.lock();
    if (dst >= dk->c->capacity || src >= sk->c->capacity) return ZRC4_ERR_SLOT_RANGE;
    int rc;
    if ((rc = sk->drain()) != ZRC4_OK) return rc;
    if (dk != sk && (rc = dk->drain()) != ZRC4_OK) return rc;
    const KsLevel S = sk->lv[src];
    if (S.lost) return ZRC4_ERR_STATE;
    const uint64_t buffered = S.gen - S.use;
    if (buffered > dk->ring) return ZRC4_ERR_INVALID_ARG;
    if (dk->c->device == sk->c->device) {
        // the state at S.gen, slot to slot on the device: two launches, one wait
        if ((rc = zrc4_copy_states(dk->c, nullptr, dst, sk->c, nullptr, src, 1, dk->c->stream)) != ZRC4_OK) return rc;
        if ((rc = check_err(dk->c, dk->c->stream)) != ZRC4_OK) return rc;
    } else {
        uint8_t sb[256], x = 0, y = 0;
        if ((rc = set_device(sk->c)) != ZRC4_OK) return rc;
        if ((rc = zrc4_get_state(sk->c, src, sb, &x, &y)) != ZRC4_OK) return rc;   // the state at S.gen
        if ((rc = set_device(dk->c)) != ZRC4_OK) return rc;
        if ((rc = zrc4_set_state(dk->c, dst, sb, x, y)) != ZRC4_OK) return rc;
    }
    dk->resetRing(dst);
    if (buffered) {
        uint8_t *sr = sk->ringOf(src), *dr = dk->ringOf(dst);
        if (!sr || !dr) return ZRC4_ERR_OUT_OF_MEMORY;
        for (uint64_t i = 0; i < buffered; ++i) dr[i] = sr[(S.use + i) % sk->ring];
        dk->lv[dst].gen = dk->lv[dst].pend = buffered;
    }
    return ZRC4_OK;
}

int zrc4_ks_stats(zrc4_ks *k, uint64_t out[6])
{
    if (!k || !out) return ZRC4_ERR_INVALID_ARG;
    std::lock_guard<std::mutex> g(k->mu);
    for (int i = 0; i < 6; ++i) out[i] = k->st[i];
    return ZRC4_OK;
}

}  // extern "C"
