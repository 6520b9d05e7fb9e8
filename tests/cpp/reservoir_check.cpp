// reservoir_check.cpp -- TEST INFRASTRUCTURE ONLY.
//
// The keystream-reservoir core (zsummerx_amd/csrc/zrc4_reservoir.hpp) alone on
// the CPU: this file defines the HIP runtime calls the core makes, with
// switches that make the n-th hipHostMalloc / hipEventRecord / hipEventQuery /
// hipEventSynchronize / hipStreamSynchronize fail, and a "launch" that stores
// oracle RC4 keystream (oracle/rc4_oracle.h) when its refill completes, not
// when it is queued -- so a byte read before its commit is the 0xA5 fill or
// stale.  Random consume / reseed sequences and each failure path in turn are
// checked against the invariants in the core's header and against the oracle
// keystream, at refill depths 1 and 2 and three ring sizes.
//
//   reservoir_check_emu [seed]     last line: {"ok": true, ...}
#include <hip/hip_runtime_api.h>

#include <cstdio>
#include <cstdlib>
#include <deque>
#include <random>
#include <vector>

#include "zrc4_reservoir.hpp"
extern "C" {
#include "rc4_oracle.h"
}

namespace {

[[noreturn]] void fail(const char *what, int line)
{
    std::printf("{\"ok\": false, \"failed\": \"%s\", \"line\": %d}\n", what, line);
    std::exit(1);
}
#define CHECK(c) ((c) ? (void)0 : fail(#c, __LINE__))

// countdowns: n > 0 makes the n-th call from now fail
struct Switches {
    int hostMalloc = 0, eventRecord = 0, eventQuery = 0, eventSync = 0, streamSync = 0, launch = 0;
} g_fail;
bool hit(int &n) { return n > 0 && --n == 0; }

// The emulated stream: launches queue their stores; a refill's stores happen
// when its event completes (or the stream is waited for).
struct Store {
    uint8_t *dst;
    std::vector<uint8_t> bytes;
};
std::deque<std::vector<Store>> g_queue;
uint64_t g_launched = 0, g_done = 0;
void runUntil(uint64_t seq)
{
    for (; g_done < seq; ++g_done) {
        for (const Store &s : g_queue.front()) std::memcpy(s.dst, s.bytes.data(), s.bytes.size());
        g_queue.pop_front();
    }
}
struct Event {
    uint64_t seq = 0;
};
unsigned g_queries = 0;
int g_stream_tag;

}  // namespace

// HIP runtime calls used by the core (C++ linkage, as hip_runtime_api.h declares them).
hipError_t hipHostMalloc(void **p, size_t n, unsigned int)
{
    *p = hit(g_fail.hostMalloc) ? nullptr : std::aligned_alloc(64, (n + 63) / 64 * 64);
    return *p ? hipSuccess : hipErrorOutOfMemory;
}
hipError_t hipHostFree(void *p)
{
    std::free(p);
    return hipSuccess;
}
hipError_t hipEventCreateWithFlags(hipEvent_t *e, unsigned)
{
    *e = reinterpret_cast<hipEvent_t>(new Event);
    return hipSuccess;
}
hipError_t hipEventDestroy(hipEvent_t e)
{
    delete reinterpret_cast<Event *>(e);
    return hipSuccess;
}
hipError_t hipEventRecord(hipEvent_t e, hipStream_t)
{
    if (hit(g_fail.eventRecord)) return hipErrorUnknown;
    reinterpret_cast<Event *>(e)->seq = g_launched;
    return hipSuccess;
}
// Alternate "not ready" / "done" so both commit paths (poll and wait) run.
hipError_t hipEventQuery(hipEvent_t e)
{
    if (hit(g_fail.eventQuery)) return hipErrorUnknown;
    if (++g_queries % 2) return hipErrorNotReady;
    runUntil(reinterpret_cast<Event *>(e)->seq);
    return hipSuccess;
}
hipError_t hipEventSynchronize(hipEvent_t e)
{
    if (hit(g_fail.eventSync)) return hipErrorUnknown;
    runUntil(reinterpret_cast<Event *>(e)->seq);
    return hipSuccess;
}
hipError_t hipStreamSynchronize(hipStream_t)
{
    if (hit(g_fail.streamSync)) return hipErrorUnknown;
    runUntil(g_launched);
    return hipSuccess;
}

namespace {

using zrc4::Reservoir;
const uint32_t kSlots[8] = {0, 5, 255, 256, 300, 511, 512, 767};   // three groups
constexpr uint32_t kCapacity = 768;

struct Model {
    Reservoir res;
    uint32_t ring, depth;
    std::vector<oracle_rc4_state> dev = std::vector<oracle_rc4_state>(kCapacity);    // the "device" states: at pend
    std::vector<oracle_rc4_state> want = std::vector<oracle_rc4_state>(kCapacity);   // the consumer's position in each slot's stream: at use
    std::vector<uint64_t> devPos = std::vector<uint64_t>(kCapacity, 0);
    std::mt19937 rng;
    uint64_t covered = 0, tails = 0, refused = 0;

    Model(uint32_t ring_, uint32_t depth_, uint32_t seed) : ring(ring_), depth(depth_), rng(seed)
    {
        CHECK(res.init(kCapacity, ring, ring / 4, depth, reinterpret_cast<hipStream_t>(&g_stream_tag),
                       hipHostMallocCoherent, 0xA5) == ZRC4_OK);
        for (uint32_t s : kSlots) seed_slot(s);
    }
    ~Model()
    {
        (void)hipStreamSynchronize(nullptr);
        CHECK(g_queue.empty());
    }
    void seed_slot(uint32_t s)
    {
        uint8_t key[16];
        for (uint8_t &b : key) b = (uint8_t)rng();
        oracle_make_sbox(&dev[s], key, sizeof key);
        want[s] = dev[s];
        devPos[s] = 0;
    }
    static void keystream(oracle_rc4_state &st, uint8_t *out, uint32_t n)
    {
        std::memset(out, 0, n);
        oracle_encryption(&st, out, (long)n);
    }

    // The owner's launch: the grouped layout is checked, then every busy
    // entry's next len keystream bytes are queued for base + off.
    int launch(const zrc4::GroupedTable &t)
    {
        if (hit(g_fail.launch)) {
            ++refused;
            return ZRC4_ERR_LAUNCH;
        }
        CHECK(t.n > 0 && t.groups.size() == (t.n + 255u) / 256u);
        std::vector<Store> job;
        uint32_t prev = 0;
        bool any = false;
        for (uint32_t e = 0; e < t.n; ++e) {
            const uint32_t id = t.ids.p[e];
            if (id == ZRC4_IDLE_SLOT) {
                CHECK(t.len.p[e] == 0 && e / 256u + 1 < t.groups.size());   // padding: never in the last bucket
                continue;
            }
            CHECK(id < kCapacity && id / 256u == t.groups[e / 256u] && t.len.p[e] > 0);
            CHECK(!any || id > prev);                                       // sorted, a slot once
            if (any && id / 256u != prev / 256u) CHECK(e % 256u == 0);      // a new bucket at every group change
            prev = id;
            any = true;
            Store st{res.base + t.off.p[e], std::vector<uint8_t>(t.len.p[e])};
            const uint8_t *r = res.ringOf(id);
            CHECK(st.dst >= r && st.dst + t.len.p[e] <= r + ring);          // inside the slot's ring
            keystream(dev[id], st.bytes.data(), t.len.p[e]);
            devPos[id] += t.len.p[e];
            job.push_back(std::move(st));
        }
        g_queue.push_back(std::move(job));
        ++g_launched;
        return ZRC4_OK;
    }
    int refill()
    {
        return res.launchRefill([this](const zrc4::GroupedTable &t) { return launch(t); }, zrc4::NoFaults());
    }

    void invariants()
    {
        size_t marked = 0;
        for (uint32_t s = 0; s < kCapacity; ++s) {
            const Reservoir::Level &L = res.level(s);
            CHECK(L.use <= L.gen && L.gen <= L.pend && L.pend - L.use <= ring);
            CHECK(devPos[s] == L.pend);
            if (L.pend > L.gen) {               // only while a refill that ends there is queued
                bool queued = false;
                for (uint32_t i = 0; i < Reservoir::kMaxDepth; ++i)
                    for (const auto &e : res.refill(i).ends) queued = queued || (e.first == s && e.second == L.pend);
                CHECK(res.inflight() > 0 && queued);
            }
            marked += res.marked(s);
        }
        CHECK(res.inflight() <= depth);
        if (!res.inflight())
            for (uint32_t i = 0; i < Reservoir::kMaxDepth; ++i) CHECK(res.refill(i).ends.empty());
        CHECK(marked == res.hungry().size());   // in the list exactly when marked (and once)
        for (uint32_t s : res.hungry()) CHECK(res.marked(s));
    }
    std::vector<Reservoir::Level> levels()
    {
        std::vector<Reservoir::Level> v;
        for (uint32_t s : kSlots) v.push_back(res.level(s));
        return v;
    }
    static bool same(const std::vector<Reservoir::Level> &a, const std::vector<Reservoir::Level> &b)
    {
        for (size_t i = 0; i < a.size(); ++i)
            if (a[i].gen != b[i].gen || a[i].use != b[i].use || a[i].pend != b[i].pend) return false;
        return true;
    }

    // One consumer call over spans (slot, len), as the owners make it.
    void consume(const std::vector<std::pair<uint32_t, uint32_t>> &spans, bool refills = true)
    {
        CHECK(res.poll(zrc4::NoFaults()) == ZRC4_OK);
        invariants();
        CHECK(res.waitCovered((uint32_t)spans.size(), [&](uint32_t i) { return spans[i]; }, zrc4::NoFaults()) == ZRC4_OK);
        invariants();
        std::vector<std::pair<uint32_t, uint32_t>> tail;
        std::vector<uint8_t> ks;
        for (const auto &sp : spans) {
            const uint32_t s = sp.first;
            const Reservoir::Level L0 = res.level(s);
            const uint8_t *r = res.ring() && L0.gen > L0.use ? res.ringOf(s) : nullptr;
            uint32_t got = 0, pieces = 0;
            const uint32_t t = res.cover(s, sp.second, [&](uint32_t done, const uint8_t *q, uint32_t m) {
                CHECK(done == got && m > 0 && ++pieces <= 2);
                CHECK(L0.use + done + m <= L0.gen);                          // inside [use, gen)
                CHECK(q == r + (L0.use + done) % ring && (L0.use + done) % ring + m <= ring);   // never across the ring end
                ks.resize(m);
                keystream(want[s], ks.data(), m);
                CHECK(std::memcmp(q, ks.data(), m) == 0);                    // the oracle's bytes at this position
                got += m;
            });
            CHECK(got + t == sp.second && res.level(s).use == L0.use + got);
            covered += got;
            if (t) tail.push_back({s, t});
            if (sp.second) res.markHungry(s);
            invariants();
        }
        if (!tail.empty()) {
            CHECK(res.drain(zrc4::NoFaults()) == ZRC4_OK);
            for (const auto &tl : tail) {
                CHECK(devPos[tl.first] == res.level(tl.first).use);          // the device state sits at use
                ks.resize(tl.second);
                keystream(dev[tl.first], ks.data(), tl.second);
                keystream(want[tl.first], ks.data(), tl.second);
                devPos[tl.first] += tl.second;
                res.afterTail(tl.first, tl.second);
                tails += tl.second;
            }
            invariants();
        }
        while (refills && res.inflight() < depth) {
            const uint32_t before = res.inflight();
            CHECK(refill() == ZRC4_OK);
            invariants();
            if (res.inflight() == before) break;
        }
    }
    void reseed(uint32_t s)
    {
        CHECK(res.drain(zrc4::NoFaults()) == ZRC4_OK);
        seed_slot(s);
        res.reset(s);
        invariants();
    }
    void randomOps(int calls)
    {
        for (int c = 0; c < calls; ++c) {
            if (rng() % 16 == 0) reseed(kSlots[rng() % 8]);
            std::vector<std::pair<uint32_t, uint32_t>> spans;
            for (uint32_t s : kSlots)
                if (rng() % 2) spans.push_back({s, rng() % 4 ? (uint32_t)(rng() % (ring / 3 + 2)) : (uint32_t)(rng() % (2 * ring))});
            std::shuffle(spans.begin(), spans.end(), rng);
            consume(spans);
        }
    }
};

// Each failure path in turn, on a fresh reservoir, then a random sequence.
void failures(uint32_t ring, uint32_t depth, uint32_t seed)
{
    {   // pinned memory exhausted at a slot's first refill, an earlier slot of the refill having its ring
        Model m(ring, depth, seed);
        m.consume({{0, 10}, {256, 10}}, false);
        const auto before = m.levels();
        g_fail.hostMalloc = 2;
        CHECK(m.refill() == ZRC4_ERR_OUT_OF_MEMORY);
        CHECK(Model::same(before, m.levels()) && m.res.inflight() == 0 && g_launched == g_done);
        m.invariants();
        g_fail.hostMalloc = 3;                  // ... and at the refill's table
        CHECK(m.refill() == ZRC4_ERR_OUT_OF_MEMORY);
        CHECK(Model::same(before, m.levels()) && m.res.inflight() == 0);
        m.invariants();
        m.randomOps(100);
    }
    {   // launch refused: pend goes back, nothing to commit
        Model m(ring, depth, seed + 1);
        m.randomOps(20);
        CHECK(m.res.drain(zrc4::NoFaults()) == ZRC4_OK);
        m.consume({{5, 3}, {300, ring}, {767, 1}}, false);
        const auto before = m.levels();
        g_fail.launch = 1;
        CHECK(m.refill() == ZRC4_ERR_LAUNCH && m.refused == 1);
        CHECK(Model::same(before, m.levels()) && m.res.inflight() == 0);
        m.invariants();
        m.randomOps(100);
    }
    {   // event not recordable: committed after the stream wait, the queue not advanced
        Model m(ring, depth, seed + 2);
        m.randomOps(20);
        CHECK(m.res.drain(zrc4::NoFaults()) == ZRC4_OK);
        m.consume({{255, ring}, {512, 9}}, false);   // (a whole ring: slot 255 has room for a chunk)
        g_fail.eventRecord = 1;
        const uint64_t launches = m.res.launches;
        CHECK(m.refill() == ZRC4_OK && m.res.launches == launches + 1 && m.res.inflight() == 0);
        CHECK(m.res.level(255).gen == m.res.level(255).pend && m.res.level(255).gen > m.res.level(255).use);
        m.invariants();
        m.consume({{0, ring}}, false);
        g_fail.eventRecord = 1;                 // ... and the stream wait fails too: an error, nothing committed
        g_fail.streamSync = 1;
        const uint64_t gen = m.res.level(0).gen;
        CHECK(m.refill() == ZRC4_ERR_HIP && m.res.level(0).gen == gen && m.res.inflight() == 0);
    }
    {   // event query / wait errors come back as errors without committing
        Model m(ring, depth, seed + 3);
        m.consume({{0, 4}, {511, 4}}, false);
        CHECK(m.refill() == ZRC4_OK && m.res.inflight() == 1);
        const auto before = m.levels();
        g_fail.eventQuery = 1;
        CHECK(m.res.poll(zrc4::NoFaults()) == ZRC4_ERR_HIP);
        CHECK(Model::same(before, m.levels()) && m.res.inflight() == 1);
        g_fail.eventSync = 1;
        CHECK(m.res.drain(zrc4::NoFaults()) == ZRC4_ERR_HIP);
        CHECK(Model::same(before, m.levels()) && m.res.inflight() == 1);
        g_fail.eventSync = 1;
        CHECK(m.res.waitCovered(1, [](uint32_t) { return std::pair<uint32_t, uint32_t>{0u, 1u}; }, zrc4::NoFaults()) == ZRC4_ERR_HIP);
        CHECK(Model::same(before, m.levels()) && m.res.inflight() == 1);
        // a fault reported by the owner's poll keeps the refill queued as well
        CHECK(m.res.drain([] { return ZRC4_ERR_GROUP; }) == ZRC4_ERR_GROUP);
        CHECK(Model::same(before, m.levels()) && m.res.inflight() == 1);
        m.invariants();
        m.randomOps(100);
    }
}

}  // namespace

int main(int argc, char **argv)
{
    const uint32_t seed = argc > 1 ? (uint32_t)std::strtoul(argv[1], nullptr, 10) : 1u;
    uint64_t covered = 0, tails = 0, launches = 0;
    for (uint32_t depth : {1u, 2u})
        for (uint32_t ring : {64u, 100u, 1000u}) {
            {
                Model m(ring, depth, seed * 977u + ring + depth);
                m.randomOps(300);
                CHECK(m.covered > 0 && m.tails > 0 && m.res.coveredBytes == m.covered);
                CHECK(m.res.drain(zrc4::NoFaults()) == ZRC4_OK && m.res.queuedBytes == m.res.committedBytes);
                covered += m.covered;
                tails += m.tails;
                launches += m.res.launches;
            }
            failures(ring, depth, seed * 31u + ring);
        }
    {   // no ring: every span is a tail, nothing is ever queued
        Model m(0, 2, seed);
        m.consume({{0, 100}, {256, 1}});
        CHECK(m.covered == 0 && m.tails == 101 && m.res.launches == 0 && m.res.hungry().empty());
    }
    std::printf("{\"ok\": true, \"seed\": %u, \"ring_bytes\": %llu, \"tail_bytes\": %llu, \"refill_launches\": %llu}\n", seed,
                (unsigned long long)covered, (unsigned long long)tails, (unsigned long long)launches);
    return 0;
}
