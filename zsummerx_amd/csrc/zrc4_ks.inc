// zrc4_ks.inc -- keystream reservoirs over a context (include/zrc4.h,
// zrc4_ks_*), included by zrc4.hip.
//
// The per-call RC4Encryption::encryption (rc4_encryption.h:74-93) of the C++
// mirror used to be one launch and one wait per call: ~15 us of round trip
// plus the serial chain of the call's bytes.  A reservoir keeps keystream the
// device generated AHEAD in pinned host rings, so a call is a host XOR and goes
// to the device only for what its ring does not cover (a "tail", e.g. a slot's
// first call after makeSBox).  The RC4 state never leaves the device and
// keystream bytes are consumed in order, so every output byte is the reference's.
//
// The levels, rings, hungry list, refill queue and their ordering rules are the
// reservoir core's (zrc4_reservoir.hpp: the design and its invariants are
// stated there), shared with the session engine's hooks
// (zsummerx_amd/engine/rc4_hooks_device.cpp).  This file adds what the C-ABI
// promises around it:
//   * a tail crypt (zrc4_crypt_host), a reseed or a state copy first drains
//     every queued refill, then resets the slot or sets gen = pend = use;
//   * a failed tail crypt loses its call's slots (ZRC4_ERR_STATE until
//     reseeded or copied into);
//   * a refill that cannot be queued is retried by the next call;
//   * the fault latch is polled before a finished refill is committed;
//   * every entry point takes the reservoir's mutex: one thread at a time per
//     reservoir (and the context's staging buffers with it).

#include <mutex>

#include "zrc4_reservoir.hpp"

struct zrc4_ks {
    zrc4_ctx *c = nullptr;
    hipStream_t sB = nullptr;
    std::mutex mu;
    zrc4::Reservoir res;
    std::vector<uint8_t> lost;            // a failed tail crypt: position unknown until reseeded or copied into
    std::vector<uint8_t> tailBuf;
    std::vector<uint32_t> tailIds, tailLen;
    std::vector<uint64_t> tailOff;
    std::vector<uint8_t *> tailDst;
    uint64_t tailBytes = 0, tailLaunches = 0;
    uint64_t refillFailures = 0;          // refills that could not be queued (retried by the next call)
    // Test hook, in ZRC4_TEST_HOOKS builds only (libzrc4_testhooks.so):
    // $ZRC4_KS_FAIL_TAIL_AFTER = n makes the n-th tail crypt of this reservoir
    // fail before launching (tests/test_gpu_parity.py: a failed call loses
    // its slots' positions -> ZRC4_ERR_STATE until reseeded).
    uint64_t failTailsAfter = 0, tailCalls = 0;

    auto faults()
    {
        return [this] { return zrc4_poll_faults(c); };
    }
    int poll() { return res.poll(faults()); }
    int drain() { return res.drain(faults()); }

    // One refill (zrc4_reservoir.hpp) as a write-only grouped launch, the path
    // of zrc4_keystream_grouped.  (The groups built by the core are declared to
    // the launch; trusted: no up-front check above 256 buckets, where they are
    // not used.)
    int launchRefill()
    {
        return res.launchRefill(
            [this](const zrc4::GroupedTable &t) {
                if (set_device(c)) return ZRC4_ERR_HIP;
                CryptCall k = crypt_call(zrc4::kGrouped, t.ids.p, 0, res.base, t.off.p, t.len.p, t.n);
                k.decl = t.groups.data();
                k.trusted = true;
                k.io = zrc4::kIoKs;
                return launch_crypt(c, k, sB);
            },
            faults());
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
        ++tailLaunches;
        return ZRC4_OK;
    }

    void resetRing(uint32_t s)
    {
        res.reset(s);
        lost[s] = 0;
    }
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
    const uint32_t chunk = ring_bytes ? std::max<uint32_t>(64u, ring_bytes / 4u) : 0u;
    k->lost.assign(c->capacity, 0);
    if (hipStreamCreateWithFlags(&k->sB, hipStreamNonBlocking) != hipSuccess ||
        k->res.init(c->capacity, ring_bytes, chunk, zrc4::Reservoir::kMaxDepth, k->sB, hipHostMallocCoherent) != ZRC4_OK) {
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
        k->res.release();
        if (k->sB) (void)hipStreamDestroy(k->sB);
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
        const zrc4::Reservoir::Level &L = k->res.level(ids[i]);
        if (k->lost[ids[i]] || L.gen < L.use) return ZRC4_ERR_STATE;
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
    rc = k->res.waitCovered(n, [&](uint32_t i) { return std::pair<uint32_t, uint32_t>(ids[i], len[i]); }, k->faults());
    if (rc != ZRC4_OK) return rc;
    k->tailIds.clear();
    k->tailLen.clear();
    k->tailOff.clear();
    k->tailDst.clear();
    k->tailBuf.clear();
    for (uint32_t i = 0; i < n; ++i) {
        const uint32_t s = ids[i];
        if (!len[i]) continue;
        const uint32_t t = k->res.cover(s, len[i], [&](uint32_t done, const uint8_t *q, uint32_t m) {
            uint8_t *d = data[i] + done;
            for (uint32_t b = 0; b < m; ++b) d[b] ^= q[b];
        });
        if (t) {
            const uint32_t have = len[i] - t;
            k->tailIds.push_back(s);
            k->tailLen.push_back(t);
            k->tailOff.push_back(k->tailBuf.size());
            k->tailDst.push_back(data[i] + have);
            k->tailBuf.insert(k->tailBuf.end(), data[i] + have, data[i] + len[i]);
            k->tailBytes += t;                   // use moves only once the tail crypt succeeded
        }
        k->res.markHungry(s);
    }
    if (!k->tailIds.empty()) {
        if ((rc = k->runTails()) != ZRC4_OK) {
            // The device may or may not have advanced the tail slots, and the
            // ring-covered spans of this call are already crypted: the call
            // fails as a whole, so every slot of it is lost (ZRC4_ERR_STATE
            // on later calls) until reseeded or copied into -- a caller
            // cannot retry part of a batch it cannot see.
            for (uint32_t i = 0; i < n; ++i)
                if (len[i]) k->lost[ids[i]] = 1;
            return rc;
        }
        for (size_t t = 0; t < k->tailIds.size(); ++t) k->res.afterTail(k->tailIds[t], k->tailLen[t]);
    }
    // Background refills are best-effort for this call: its bytes are already
    // crypted, so a refill that cannot be queued now (pinned-memory or launch
    // failure) is retried by the next call, which crypts on the device what
    // the rings then lack.  Hard errors are reserved for the tail path.
    while (k->res.inflight() < zrc4::Reservoir::kMaxDepth) {
        const uint32_t before = k->res.inflight();
        if (k->launchRefill() != ZRC4_OK) {
            ++k->refillFailures;
            break;
        }
        if (k->res.inflight() == before) break;
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
    const zrc4::Reservoir::Level S = sk->res.level(src);
    if (sk->lost[src]) return ZRC4_ERR_STATE;
    const uint64_t buffered = S.gen - S.use;
    if (buffered > dk->res.ring()) return ZRC4_ERR_INVALID_ARG;
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
        uint8_t *sr = sk->res.ringOf(src), *dr = dk->res.ringOf(dst);
        if (!sr || !dr) return ZRC4_ERR_OUT_OF_MEMORY;
        for (uint64_t i = 0; i < buffered; ++i) dr[i] = sr[(S.use + i) % sk->res.ring()];
        dk->res.reset(dst, buffered);
    }
    return ZRC4_OK;
}

int zrc4_ks_stats(zrc4_ks *k, uint64_t out[6])
{
    if (!k || !out) return ZRC4_ERR_INVALID_ARG;
    std::lock_guard<std::mutex> g(k->mu);
    // ring bytes, tail bytes, tail launches, refill bytes (queued), refill launches, refill waits
    const uint64_t st[6] = {k->res.coveredBytes, k->tailBytes, k->tailLaunches,
                            k->res.queuedBytes, k->res.launches, k->res.waits};
    for (int i = 0; i < 6; ++i) out[i] = st[i];
    return ZRC4_OK;
}

}  // extern "C"
