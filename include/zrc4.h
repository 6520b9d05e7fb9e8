/*
 * zrc4.h -- C-ABI of the MI355X-native RC4 payload-encryption path for
 * zsummerX (the drop-in behind SessionOptions::_rc4TcpEncryption).
 *
 * Reference interface this boundary replaces
 * (/root/reference, read-only):
 *   class RC4Encryption                      depends/rc4/rc4_encryption.h:43-99
 *     void makeSBox(std::string obscure)     depends/rc4/rc4_encryption.h:46-72
 *     void encryption(unsigned char*, int)   depends/rc4/rc4_encryption.h:74-93
 *     int _x, _y, _box[256]                  depends/rc4/rc4_encryption.h:96-98
 *   reached only from TcpSession:
 *     seeding  _rc4StateRead/_rc4StateWrite.makeSBox   src/frame/session.cpp:110-111
 *     decrypt  _rc4StateRead.encryption(recv tail)     src/frame/session.cpp:313-323
 *     encrypt  _rc4StateWrite.encryption(_sending)     src/frame/session.cpp:496-499,
 *                                                      535-538, 603-606
 *   switch    SessionOptions::_rc4TcpEncryption (empty = off)
 *                                                      include/zsummerX/frame/config.h:196
 *
 * Model.  A context owns one device (HIP/gfx950) and a device-resident arena of
 * `capacity` RC4 streams ("slots"; a TcpSession owns two: read and write).  A
 * slot's state is the reference state (S-box + x + y) held as 258 bytes.  The
 * batched entry points take DEVICE pointers and are stream-ordered and
 * asynchronous; the *_host entry points take host pointers and block.
 *
 * Conventions (all functions):
 *   - return 0 (ZRC4_OK) or a negative ZRC4_ERR_* code; nothing throws across
 *     the ABI; zrc4_strerror() names a code.
 *   - ids == NULL means the identity map (batch entry i -> slot i).
 *   - a slot may appear at most once per call; len == 0 is a no-op for that
 *     slot (reference: `length <= 0` never enters the loop, :81).
 *   - every `base + off` (payload + off[i], keys + key_off[i], src + src_off[i],
 *     dst + dst_off[i], frame->off[i], ring + rid * ring_cap) is computed
 *     modulo 2^64, so an offset may be the two's-complement difference of an
 *     address BELOW the base: one base pointer serves spans anywhere in the
 *     address space, on either side of it and of any multiple of 2^32.
 *   - calls on one context are serialised by the caller (one event-loop
 *     thread, as the reference: include/zsummerX/frame/manager.h:98-110);
 *     concurrent calls on different streams must touch disjoint 256-slot
 *     groups (slot / 256).
 *   - no CPU fallback: with no usable gfx950 device zrc4_create fails with
 *     ZRC4_ERR_NO_DEVICE.
 *   - device-side faults of a batched call (a slot id >= capacity) are latched
 *     and reported by the next zrc4_sync() as ZRC4_ERR_SLOT_RANGE; the affected
 *     entries are skipped (caller closes those sessions, as the reference does
 *     on BCT_CORRUPTION, src/frame/session.cpp:355-361).  The latch belongs to
 *     the CONTEXT, not to a stream: zrc4_sync on any stream reports (and
 *     clears) faults of every kernel of the context that has completed, so a
 *     caller that uses several streams syncs them all before acting on a
 *     fault.
 */
#ifndef ZRC4_H
#define ZRC4_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define ZRC4_OK 0
#define ZRC4_ERR_INVALID_ARG (-1)
#define ZRC4_ERR_NO_DEVICE (-2)
#define ZRC4_ERR_OUT_OF_MEMORY (-3)
#define ZRC4_ERR_LAUNCH (-4)
#define ZRC4_ERR_SLOT_RANGE (-5)
#define ZRC4_ERR_HIP (-6)
#define ZRC4_ERR_GROUP (-7)    /* zrc4_crypt_grouped: a bucket broke the bucket contract */
#define ZRC4_ERR_INTERNAL (-8) /* kernel self-check failed (LDS layout) */
#define ZRC4_ERR_STATE (-9)    /* zrc4_ks_crypt / zrc4_ks_copy: the slot's stream position
                                  was lost by a failed zrc4_ks_crypt; reseed it
                                  (zrc4_ks_make_sbox) or copy into it (zrc4_ks_copy) */

/* Slots are grouped 256 to a 64 KiB device image (the LDS image of one
 * workgroup); capacity is rounded up to a multiple of this. */
#define ZRC4_GROUP_SLOTS 256u
#define ZRC4_STATE_BYTES 258u

typedef struct zrc4_ctx zrc4_ctx;

/* Create a context on HIP device `device` with room for `capacity` streams.
 * Replaces: the per-session RC4Encryption members (session.h:115-116). */
int zrc4_create(zrc4_ctx **out, int device, uint32_t capacity);
int zrc4_destroy(zrc4_ctx *ctx);
uint32_t zrc4_capacity(const zrc4_ctx *ctx);

/* Batched KSA (RC4Encryption::makeSBox, rc4_encryption.h:46-72) for n slots.
 * Entry i seeds slot ids[i] from keys[key_off[i] .. key_off[i]+key_len[i]);
 * key bytes may be NUL; key_len 0 gives the identity S-box with x = y = 0.
 * Device pointers; asynchronous on `stream` (hipStream_t, NULL = default). */
int zrc4_ksa(zrc4_ctx *ctx, const uint32_t *ids, const uint8_t *keys,
             const uint64_t *key_off, const uint32_t *key_len, uint32_t n,
             void *stream);

/* Batched PRGA+XOR (RC4Encryption::encryption, rc4_encryption.h:74-93), in
 * place: entry i crypts payload[off[i] .. off[i]+len[i]) with slot ids[i] and
 * advances that slot by len[i] bytes.  Device pointers; asynchronous. */
int zrc4_crypt(zrc4_ctx *ctx, const uint32_t *ids, uint8_t *payload,
               const uint64_t *off, const uint32_t *len, uint32_t n,
               void *stream);

/* Contiguous-slot variants: entry i uses slot first_slot + i (no ids array).
 * When first_slot is a multiple of 256 every workgroup owns a whole slot
 * group and moves its state as one coalesced 64 KiB image: the fast path for
 * a session engine that allocates its streams in groups.  Requires
 * first_slot + n <= capacity.  Device pointers; asynchronous. */
int zrc4_ksa_range(zrc4_ctx *ctx, uint32_t first_slot, const uint8_t *keys,
                   const uint64_t *key_off, const uint32_t *key_len, uint32_t n,
                   void *stream);
int zrc4_crypt_range(zrc4_ctx *ctx, uint32_t first_slot, uint8_t *payload,
                     const uint64_t *off, const uint32_t *len, uint32_t n,
                     void *stream);

/* Grouped-ids variant: the fast path for arbitrary slot subsets.  Entries
 * are taken in buckets of 256 (bucket b = entries [256b, 256b + 256)); the
 * caller promises that every busy entry (len > 0) of a bucket uses a slot of
 * ONE 256-slot group (slot / 256), that no other bucket of the call touches
 * that group, and that a slot appears at most once.  Entries may come in any
 * order; padding entries carry ids[i] = ZRC4_IDLE_SLOT or len 0.  Each bucket
 * then moves its group's state as one coalesced 64 KiB image, exactly like a
 * whole-group zrc4_crypt_range.  Refusals, reported by zrc4_sync as
 * ZRC4_ERR_GROUP (no payload byte, S-box or x/y of a refused bucket is
 * touched; every other bucket runs):
 *   - a bucket whose busy entries span two groups, or name a slot twice;
 *   - a bucket naming a group another bucket of the same call holds: every
 *     workgroup claims the PART of its bucket's group it moves (a dword
 *     column on the window kernel, <= 32 buckets; a half on the half-group
 *     and persistent kernels; the whole group otherwise), and the first
 *     claimant of a part runs.  Claims and refusals therefore apply per part:
 *     two buckets naming one group may each run some parts of it (each slot
 *     is still all or nothing: crypted with its state advanced, or untouched).
 *     Where the claim is taken: the window kernel (<= 32 buckets) claims
 *     only after its bucket's table check has passed, so a bucket it
 *     refuses claims nothing.  The half- and whole-group kernels (at most
 *     one bucket per CU) claim while the check runs, on the bucket's first
 *     busy id (zrc4_crypt_grouped_declared: on the declared group), and the
 *     persistent kernel (more buckets than CUs) claims a bucket's group
 *     before its slot table can refuse a slot named twice.  So on those
 *     kernels a bucket that breaks the one-group or once-per-slot rule may
 *     also block a valid bucket of a group it names.
 * An id >= capacity other than ZRC4_IDLE_SLOT is skipped and reported as
 * ZRC4_ERR_SLOT_RANGE (the rest of its bucket runs).  The claims carry a
 * per-call tag chosen on the host: a grouped call must not be captured into
 * a HIP graph and replayed (the replay would find its own tags and refuse
 * every bucket).  n <= 0xFFF00000.  Device pointers; asynchronous. */
#define ZRC4_IDLE_SLOT 0xFFFFFFFFu
int zrc4_crypt_grouped(zrc4_ctx *ctx, const uint32_t *ids, uint8_t *payload,
                       const uint64_t *off, const uint32_t *len, uint32_t n,
                       void *stream);

/* zrc4_crypt_grouped with each bucket's group declared by the caller, who
 * built the buckets on the host and so already knows them (the session
 * engine, zrc4_crypt_host).  bucket_group is HOST memory of ceil(n / 256)
 * entries, read during the call: bucket b's group (slot / 256 of its busy
 * entries), or ZRC4_IDLE_SLOT for a bucket with no busy entry.  A group
 * >= capacity / 256 returns ZRC4_ERR_INVALID_ARG and launches nothing.
 * Semantics are zrc4_crypt_grouped's, plus one refusal: a bucket with a busy
 * entry outside its declared group is refused (ZRC4_ERR_GROUP, nothing of it
 * written).  Why: with at most 256 buckets (at most one bucket per CU, where
 * the launch is one keystream chain long) the groups travel in the kernel
 * arguments, so each bucket's state image is loaded with its entries instead
 * of after a dependent read of the bucket's ids.  With more buckets the
 * declared groups are checked by a short kernel on the same stream just
 * before the crypt launch (it reads them from pinned memory the call fills);
 * a disagreeing bucket's own ids then also block the groups they name, so
 * another bucket naming one of those groups is refused too (the rule for two
 * buckets naming one group).  Callers that build their buckets themselves
 * gain nothing from the declaration above 256 buckets: there the persistent
 * kernel already prefetches each bucket's ids a bucket ahead.  frame: NULL for
 * no framing, else zrc4_crypt_grouped_frame's framing (below).  Device
 * pointers apart from bucket_group; asynchronous. */
struct zrc4_frame_args;
int zrc4_crypt_grouped_declared(zrc4_ctx *ctx, const uint32_t *ids,
                                const uint32_t *bucket_group, uint8_t *payload,
                                const uint64_t *off, const uint32_t *len,
                                uint32_t n, const struct zrc4_frame_args *frame,
                                void *stream);

/* Write-only keystream: zrc4_crypt_range / zrc4_crypt_grouped with one
 * difference: entry i STORES the next len[i] keystream bytes of its slot into
 * out[off[i] .. off[i]+len[i]) and advances the slot by len[i] bytes.  The
 * previous contents of `out` are never read (no zeroing by the caller, no
 * load of the destination: what a keystream reservoir refills its rings
 * with).  Everything else is the crypt calls': the slot rules, the bucket
 * contract, the claims and their per-part refusals, n <= 0xFFF00000, no
 * capture into a replayed HIP graph, disjoint 256-slot groups for concurrent
 * streams, and the faults latched for zrc4_sync.  bucket_group: NULL, or HOST
 * memory with zrc4_crypt_grouped_declared's meaning and rules (a group >=
 * capacity / 256 returns ZRC4_ERR_INVALID_ARG and launches nothing).
 *   - bytes outside the spans are not written;
 *   - the span of a skipped entry (ids[i] == ZRC4_IDLE_SLOT, len[i] == 0, or
 *     an id >= capacity, reported as ZRC4_ERR_SLOT_RANGE) is left untouched;
 *   - the spans of a bucket refused with ZRC4_ERR_GROUP are unspecified:
 *     untouched or zero.  Its slots' states are untouched.
 *   - launches of at most one group or bucket per CU leave a refused bucket's
 *     spans untouched: the kernels return, or lose their claim, before their
 *     first store, as in the in-place calls (zero shows only behind the
 *     zeroing launch below).
 * `out` is device memory or coherent pinned host memory, at any alignment
 * (16-byte aligned span starts store whole 16-byte units).  With at most one
 * group or bucket per CU the kernels store the keystream themselves, in one
 * launch.  With more (the persistent throughput kernel, which has no
 * write-only form) the call makes TWO launches on `stream`: a short kernel
 * that zeroes the span of every entry that is not skipped, then the crypt
 * launch over the zeroed spans (0 ^ k = k); the destination is then written
 * twice and read once, by the device only.  There are no _host or _frame
 * variants.  Device pointers apart from bucket_group; asynchronous. */
int zrc4_keystream_range(zrc4_ctx *ctx, uint32_t first_slot, uint8_t *out,
                         const uint64_t *off, const uint32_t *len, uint32_t n,
                         void *stream);
int zrc4_keystream_grouped(zrc4_ctx *ctx, const uint32_t *ids,
                           const uint32_t *bucket_group, uint8_t *out,
                           const uint64_t *off, const uint32_t *len, uint32_t n,
                           void *stream);

/* Out-of-place crypt with shared sources (broadcast encrypt): zrc4_crypt_range
 * / zrc4_crypt_grouped with one difference: entry i reads a SOURCE span and
 * writes a DESTINATION span.  It stores src[src_off[i]+k] ^ keystream_i[k]
 * into dst[dst_off[i]+k] for k < len[i] and advances its slot by len[i] bytes.
 * One message for N sessions is N entries with the same src_off: the
 * plaintext is read N times (from cache) and never copied.  Everything else is
 * the crypt calls': the slot rules, the bucket contract, the claims and their
 * per-part refusals, n <= 0xFFF00000, no capture into a replayed HIP graph,
 * disjoint 256-slot groups for concurrent streams, and the faults latched for
 * zrc4_sync.  bucket_group: NULL, or HOST memory with
 * zrc4_crypt_grouped_declared's meaning and rules (a group >= capacity / 256
 * returns ZRC4_ERR_INVALID_ARG and launches nothing).
 *   - `src` is never written;
 *   - bytes of `dst` outside the spans are never written;
 *   - a destination span is never read, except that an entry whose source
 *     and destination are the SAME ADDRESS is exactly the in-place crypt;
 *   - source spans may overlap each other freely (the same span N times,
 *     prefixes of one message, anything);
 *   - a destination span must not overlap another entry's destination span;
 *   - a destination span must not overlap any source span other than its own
 *     identical one; partial overlap of an entry's own two spans is undefined;
 *   - the span of a skipped entry (ids[i] == ZRC4_IDLE_SLOT, len[i] == 0, or
 *     an id >= capacity, reported as ZRC4_ERR_SLOT_RANGE) is left untouched
 *     in `dst`;
 *   - the destination spans of a bucket refused with ZRC4_ERR_GROUP are
 *     unspecified: untouched, or a plain copy of the source, never partly
 *     crypted.  Its slots' states are untouched;
 *   - launches of at most one group or bucket per CU leave a refused bucket's
 *     spans untouched: the claim is answered before the first store, as in
 *     the in-place calls.
 * `src` and `dst` are device memory or coherent pinned host memory, at any
 * alignment.  On the lane-per-stream kernels (more than 32 groups or buckets)
 * and in the copy launch below every entry stores aligned 16-byte units
 * wherever the destination's alignment allows (the in-place walk); an entry
 * whose two addresses are not congruent mod 16 feeds them with 16-byte loads
 * at unaligned source addresses, which touch exactly the source span's bytes.
 * On the window kernel (at most 32) such an entry is crypted byte by byte, 16
 * lanes storing 16 adjacent bytes (DESIGN.md §14 has the numbers of both).
 * With at most one group or bucket per CU the kernels read
 * the sources themselves, in one launch.  With more (the persistent
 * throughput kernel, which has no out-of-place form) the call makes TWO
 * launches on `stream`: a short kernel that copies the source span of every
 * entry that is not skipped into its destination span (entries whose two
 * addresses are identical are left alone), then the in-place crypt launch over
 * `dst`; the destination is then written twice and read once, by the device
 * only.  There are no _host, _frame or scattered-ids (zrc4_crypt) variants.
 * Device pointers apart from bucket_group; asynchronous. */
int zrc4_crypt_to_range(zrc4_ctx *ctx, uint32_t first_slot,
                        const uint8_t *src, const uint64_t *src_off,
                        uint8_t *dst, const uint64_t *dst_off,
                        const uint32_t *len, uint32_t n, void *stream);
int zrc4_crypt_to_grouped(zrc4_ctx *ctx, const uint32_t *ids, const uint32_t *bucket_group,
                          const uint8_t *src, const uint64_t *src_off,
                          uint8_t *dst, const uint64_t *dst_off,
                          const uint32_t *len, uint32_t n, void *stream);

/* Multi-round out-of-place crypt: several spans per slot in one launch.  The
 * call behaves exactly like `rounds` successive zrc4_crypt_to_range /
 * zrc4_crypt_to_grouped calls on the same slots, round r given the tables
 * advanced by r * n: for every slot that runs, the bytes written to `dst` and
 * the final state are those.  The group image is loaded once and stored once.
 *   - src_off, dst_off and len hold rounds * n entries, ROUND-MAJOR: entry i
 *     of round r is at index r * n + i.  ids (n entries) and bucket_group
 *     (ceil(n / 256) entries, host memory) are the same for every round;
 *   - len[r*n+i] == 0 skips that round for that slot only;
 *   - an entry-round whose source and destination are the SAME ADDRESS is the
 *     in-place crypt, so "queued bytes in place, then a broadcast" is a
 *     2-round call and K broadcasts in one tick are a K-round call;
 *   - decided ONCE PER LAUNCH from ids, not per round: the skipped entries
 *     (ids[i] == ZRC4_IDLE_SLOT, or an id >= capacity, latched as
 *     ZRC4_ERR_SLOT_RANGE: skipped in every round), the bucket contract, the
 *     claims, and the refusals with ZRC4_ERR_GROUP.  A bucket is judged busy
 *     by its ids, as a one-round call with every len nonzero would judge it
 *     (a bucket declared idle that names a slot is refused even if all its
 *     lengths are zero).  Launches of at most one bucket per CU leave a
 *     refused bucket's destination spans untouched in every round, and its
 *     states untouched;
 *   - the span rules of zrc4_crypt_to_* hold over the union of ALL rounds: the
 *     destination spans of the call are pairwise disjoint; no destination
 *     overlaps any source span of the call other than an entry-round's own
 *     identical one; sources overlap freely;
 *   - rounds == 0, rounds > ZRC4_MAX_ROUNDS or (uint64_t)n * rounds >
 *     0xFFF00000: ZRC4_ERR_INVALID_ARG, nothing launched.  n == 0: ZRC4_OK.
 *     rounds == 1 is the existing call (forwarded to it).
 * Everything else is zrc4_crypt_to_*'s: device or coherent pinned memory at
 * any alignment, every entry-round stores aligned 16-byte units (fed by
 * unaligned loads where its two addresses are not congruent mod 16), no
 * capture into a replayed HIP graph, disjoint
 * 256-slot groups for concurrent streams, faults latched for zrc4_sync.
 * Kernels: with at most one group or bucket per CU the call is ONE launch of
 * the half-group, whole-group or declared kernel -- at 32 groups and fewer
 * too, where the one-round calls use the 16-lanes-per-stream window kernel,
 * which has no rounds form: there a round costs its bytes at the lane-per-
 * stream rate, and `rounds` separate calls are FASTER once messages are long.
 * Measured on MI355X at 16 buckets: one call took 0.51-0.70
 * of the separate calls' time at 64-128 bytes per message, the same at 256,
 * 1.35 times at 512 and 1.66-1.69 times at 1 KiB in device memory (1.19 times
 * into pinned host memory), 2.1 times at 4 KiB; at 32 buckets 0.82 at 256
 * bytes and 1.23 times at 1 KiB.  With at most 32 buckets and messages of
 * more than about 256 bytes keep separate calls.  With MORE groups than CUs the
 * persistent kernel has no out-of-place form, and the call issues `rounds`
 * successive two-launch zrc4_crypt_to_* sequences on `stream` from a host
 * loop: nothing is saved over separate calls, the claims are taken PER ROUND
 * (two buckets naming one group may split differently in different rounds),
 * and each slot is all-or-nothing per round, not per call.  Every round is
 * there JUDGED as a one-round call, by that round's lengths: a slot named a
 * second time with length 0 is allowed and its bucket runs, and a bucket whose
 * lengths are all zero is idle in that round (declared idle or not, it is not
 * refused), where the one-launch call above refuses both.
 * Device pointers apart from bucket_group; asynchronous. */
#define ZRC4_MAX_ROUNDS 64u
int
zrc4_crypt_to_range_rounds(zrc4_ctx *ctx, uint32_t first_slot,
                           const uint8_t *src, const uint64_t *src_off,
                           uint8_t *dst, const uint64_t *dst_off,
                           const uint32_t *len, uint32_t n, uint32_t rounds, void *stream);
int
zrc4_crypt_to_grouped_rounds(zrc4_ctx *ctx, const uint32_t *ids, const uint32_t *bucket_group,
                             const uint8_t *src, const uint64_t *src_off,
                             uint8_t *dst, const uint64_t *dst_off,
                             const uint32_t *len, uint32_t n, uint32_t rounds, void *stream);

/* Host-pointer variants: copy to the device (pinned staging), run, copy back,
 * block until done.  payload_bytes bounds the host payload buffer.
 * zrc4_crypt_host checks every id on the host first: an id >= capacity
 * (ZRC4_IDLE_SLOT included) returns ZRC4_ERR_SLOT_RANGE and crypts nothing.
 * With several ids it buckets them by group itself and runs the
 * zrc4_crypt_grouped path (a slot may appear once per call: a repeated slot
 * returns ZRC4_ERR_INVALID_ARG and crypts nothing). */
int zrc4_ksa_host(zrc4_ctx *ctx, const uint32_t *ids, const uint8_t *keys,
                  size_t keys_bytes, const uint64_t *key_off,
                  const uint32_t *key_len, uint32_t n);
int zrc4_crypt_host(zrc4_ctx *ctx, const uint32_t *ids, uint8_t *payload,
                    size_t payload_bytes, const uint64_t *off,
                    const uint32_t *len, uint32_t n);

/* Single-stream drop-ins with the reference's exact argument meaning:
 *   zrc4_make_sbox  == RC4Encryption::makeSBox(std::string(key, keylen))
 *   zrc4_encryption == RC4Encryption::encryption(data, length) (host data,
 *                      in place, length <= 0 is a no-op) */
int zrc4_make_sbox(zrc4_ctx *ctx, uint32_t id, const uint8_t *key,
                   size_t keylen);
int zrc4_encryption(zrc4_ctx *ctx, uint32_t id, uint8_t *data, int length);

/* Keystream reservoirs (the session engine's low-latency hook path,
 * zsummerx_amd/engine/rc4_hooks_device.cpp).  RC4's keystream does not depend
 * on the data, so a slot's keystream can be generated ahead into a device
 * ring of ring_cap bytes (ring r at ring + r * ring_cap): by
 * zrc4_keystream_range / zrc4_keystream_grouped (above) whatever the ring
 * holds, or by zrc4_crypt over ZEROED ring bytes (0 ^ k = k; the slot's state
 * advances as usual).
 * zrc4_xor_ring then XORs entry i's payload[off[i] .. off[i]+len[i]) with
 * ring rid[i] from position pos[i] on (wrapping mod ring_cap) and zeroes the
 * ring bytes it used.  Requires len[i] <= ring_cap and pos[i] < ring_cap; the
 * caller tracks which ring bytes hold keystream.  Device (or pinned host)
 * pointers; asynchronous on `stream`.  Touches no slot state. */
int zrc4_xor_ring(zrc4_ctx *ctx, uint8_t *ring, uint32_t ring_cap,
                  const uint32_t *rid, const uint32_t *pos, uint8_t *payload,
                  const uint64_t *off, const uint32_t *len, uint32_t n,
                  void *stream);

/* Device-side proto4z framing of decrypted session buffers (the step after
 * the recv decrypt, src/frame/session.cpp:329-371, with HasRawPacket,
 * depends/proto4z/proto4z.h:704-748, as the check): entry i walks
 * buf[off[i] .. off[i]+len[i]) from its start with the reference's
 * check(begin+used, len-used, bound-used, bound) until it stops, and writes
 *   npk[i]     complete packets found,
 *   used[i]    bytes they cover (the reference memmoves the rest down),
 *   status[i]  1 = stopped on shortage, 2 = on corruption (close the session),
 *   pkt_len[i * max_packets + k]  the first max_packets packet lengths
 *              (pkt_len may be NULL when max_packets == 0).
 * bound is the receive block size (SESSION_BLOCK_SIZE = 20480 in the
 * reference, config.h:100).  Device pointers; asynchronous on `stream`. */
int zrc4_frame_scan(zrc4_ctx *ctx, const uint8_t *buf, const uint64_t *off,
                    const uint32_t *len, uint32_t bound, uint32_t n,
                    uint32_t max_packets, uint32_t *npk, uint32_t *used,
                    uint32_t *status, uint32_t *pkt_len, void *stream);

/* Decrypt + frame in ONE launch (the recv hook followed by onRecv's framing
 * loop, src/frame/session.cpp:313-371): zrc4_crypt_range / zrc4_crypt_grouped
 * semantics for the crypt, then for every entry i the zrc4_frame_scan walk of
 * payload[frame->off[i] .. frame->off[i] + frame->len[i]) (the whole receive
 * block, which may start before the decrypted tail) into npk/used/status/
 * pkt_len[i] exactly as zrc4_frame_scan defines them.  One launch at every
 * size: in the chain-bound regime (at most one slot group per CU) each lane
 * frames its own session in the crypt kernel's epilogue; larger batches run
 * the persistent throughput kernel, whose workgroups frame the entries of the
 * 256-entry chunks they decrypted in their tail.  Framing outputs of a bucket
 * refused with ZRC4_ERR_GROUP are unspecified, with one guarantee on launches
 * of at most one bucket per CU (the window, half- and whole-group kernels,
 * declared or not): its busy entries (the ones it would have decrypted) are
 * never framed over their undecrypted bytes.  (The persistent kernel's tail
 * walks every chunk, a refused bucket's included, on its bytes as they
 * stand.)  Device pointers; asynchronous. */
typedef struct zrc4_frame_args {
    const uint64_t *off;
    const uint32_t *len;
    uint32_t bound;
    uint32_t max_packets;
    uint32_t *npk;
    uint32_t *used;
    uint32_t *status;
    uint32_t *pkt_len;
} zrc4_frame_args;
int zrc4_crypt_range_frame(zrc4_ctx *ctx, uint32_t first_slot, uint8_t *payload,
                           const uint64_t *off, const uint32_t *len, uint32_t n,
                           const zrc4_frame_args *frame, void *stream);
int zrc4_crypt_grouped_frame(zrc4_ctx *ctx, const uint32_t *ids, uint8_t *payload,
                             const uint64_t *off, const uint32_t *len, uint32_t n,
                             const zrc4_frame_args *frame, void *stream);

/* Keystream reservoir over a context (the C++ mirror's per-call path):
 * per-slot rings of ring_bytes in pinned host memory that the device fills
 * ahead with the slot's keystream (background stream, one write-only grouped
 * launch -- zrc4_keystream_grouped's path -- for every slot used since the
 * last refill; consumed ring bytes keep their keystream until a later refill
 * overwrites them).  zrc4_ks_crypt XORs host spans with
 * committed ring bytes on the host and crypts only what the rings do not
 * cover on the device, so steady-state calls make no GPU round trip; output
 * bytes are exactly RC4Encryption::encryption's.  Once a slot is used through
 * a reservoir, every state change of it must go through the same reservoir
 * (its device state runs ahead of its stream position by the buffered bytes):
 * zrc4_ks_make_sbox == makeSBox, zrc4_ks_copy == copying the RC4Encryption
 * value (device state + buffered keystream).  ring_bytes 0: no buffering
 * (every call crypts on the device).  Thread-safe per reservoir; a slot at
 * most once per zrc4_ks_crypt call.  stats: ring bytes, tail bytes, tail
 * launches, refill bytes, refill launches, refill waits.
 * Failure: a zrc4_ks_crypt whose device tail fails returns the error and
 * leaves EVERY slot of that call lost (some spans may already be crypted
 * from their rings, some not): zrc4_ks_crypt and zrc4_ks_copy return
 * ZRC4_ERR_STATE for them until zrc4_ks_make_sbox reseeds a slot or
 * zrc4_ks_copy copies a live one into it; the call's data must be treated as
 * consumed, not retried. */
typedef struct zrc4_ks zrc4_ks;
int zrc4_ks_create(zrc4_ctx *ctx, uint32_t ring_bytes, zrc4_ks **out);
int zrc4_ks_destroy(zrc4_ks *ks);
int zrc4_ks_crypt(zrc4_ks *ks, const uint32_t *ids, uint8_t *const *data,
                  const uint32_t *len, uint32_t n);
int zrc4_ks_make_sbox(zrc4_ks *ks, uint32_t id, const uint8_t *key,
                      size_t keylen);
int zrc4_ks_copy(zrc4_ks *dst_ks, uint32_t dst, zrc4_ks *src_ks, uint32_t src);
int zrc4_ks_stats(zrc4_ks *ks, uint64_t out[6]);

/* Wait for `stream`, then report (and clear) any latched device-side fault. */
int zrc4_sync(zrc4_ctx *ctx, void *stream);

/* Report (and clear) faults latched by kernels that have already completed
 * (e.g. after an event query succeeded), without waiting for any stream. */
int zrc4_poll_faults(zrc4_ctx *ctx);

/* Export / import one slot's state: S-box bytes + x + y (the reference's
 * int _box[256], _x, _y narrowed to bytes; values are always in [0,255]). */
int zrc4_get_state(zrc4_ctx *ctx, uint32_t id, uint8_t sbox[256], uint8_t *x,
                   uint8_t *y);
int zrc4_set_state(zrc4_ctx *ctx, uint32_t id, const uint8_t sbox[256],
                   uint8_t x, uint8_t y);
/* Bulk export of slots [first_slot, first_slot + n): sbox[256 i .. 256 i +
 * 255], x[i], y[i] for slot first_slot + i (host memory; blocks).  One copy of
 * the groups' images instead of a strided copy per slot (checkpointing the
 * sessions of a shard, the parity tests' state checks). */
int zrc4_get_states(zrc4_ctx *ctx, uint32_t first_slot, uint32_t n,
                    uint8_t *sbox, uint8_t *x, uint8_t *y);

/* Batched device-side export / import of states as RECORDS, and slot-to-slot
 * copy (checkpoint and restore of a shard, session migration between
 * contexts, arena compaction, copying an RC4Encryption value).
 *
 * Record i is sbox[256 i + k] = S[k] (k = 0..255) and xy[i] = x | y << 8: the
 * values zrc4_get_states returns and the arena's own x/y word.  sbox and xy
 * are DEVICE pointers (sbox 16-byte aligned, xy 2-byte aligned, else
 * ZRC4_ERR_INVALID_ARG); the calls are stream-ordered and asynchronous.
 *
 * Entry i names slot ids[i], or first_slot + i when ids is NULL (then
 * first_slot + n <= capacity, else ZRC4_ERR_SLOT_RANGE with nothing
 * launched).  n == 0 returns ZRC4_OK.  An entry with ids[i] ==
 * ZRC4_IDLE_SLOT is skipped: an export leaves its record untouched.  Any
 * other id >= capacity is skipped too and reported by zrc4_sync as
 * ZRC4_ERR_SLOT_RANGE; the rest of the call runs.
 *
 * zrc4_import_states changes only the bytes of the slots it names: every
 * other slot of a touched group keeps its state.  A slot named twice ends
 * with unspecified bytes of its two records; no other slot is affected.  With
 * ids == NULL a partly covered group is read, merged and written back as a
 * whole image, so the rule on concurrent streams and disjoint groups (top of
 * this file) applies as for every call that moves a group.
 *
 * zrc4_copy_states copies entry i's source slot (src_ids / src_first in src)
 * to its destination slot (dst_ids / dst_first in dst).  Both contexts must
 * be on the same device (else ZRC4_ERR_INVALID_ARG); dst == src is allowed.
 * Every source is read before any destination is written, so overlapping
 * ranges and permutations are well defined.  An entry is skipped when either
 * of its ids is skipped (a source id >= capacity is latched on src, a
 * destination id on dst).  The records pass through a device scratch of
 * n * 258 bytes owned by dst, grown on demand (the stream is waited for
 * first) and kept; if it cannot be had: ZRC4_ERR_OUT_OF_MEMORY, nothing
 * launched.  Copies into one destination context share that scratch: a copy
 * issued on another stream than the previous one first waits (on the device)
 * for the previous copy to finish.
 *
 * zrc4_set_states is the blocking host mirror of zrc4_get_states: host
 * pointers, slots [first_slot, first_slot + n).
 *
 * These calls move the DEVICE state as it stands.  A slot driven through a
 * keystream reservoir (zrc4_ks) runs ahead of its stream position by the
 * bytes its ring holds, so such slots are copied with zrc4_ks_copy, which
 * moves the buffered keystream along (and uses zrc4_copy_states underneath
 * when both reservoirs' contexts are on one device).
 *
 * Between two GPUs: zrc4_export_states on the source context, a peer copy of
 * the records (hipMemcpyPeerAsync), zrc4_import_states on the other context
 * ("Moving sessions"). */
int zrc4_export_states(zrc4_ctx *ctx, const uint32_t *ids, uint32_t first_slot,
                       uint32_t n, uint8_t *sbox, uint16_t *xy, void *stream);
int zrc4_import_states(zrc4_ctx *ctx, const uint32_t *ids, uint32_t first_slot,
                       uint32_t n, const uint8_t *sbox, const uint16_t *xy,
                       void *stream);
int zrc4_copy_states(zrc4_ctx *dst, const uint32_t *dst_ids, uint32_t dst_first,
                     zrc4_ctx *src, const uint32_t *src_ids, uint32_t src_first,
                     uint32_t n, void *stream);
int zrc4_set_states(zrc4_ctx *ctx, uint32_t first_slot, uint32_t n,
                    const uint8_t *sbox, const uint8_t *x, const uint8_t *y);

const char *zrc4_strerror(int code);
const char *zrc4_version(void);   /* a non-product build appends " [KNOB=value]" per build knob set */

#ifdef __cplusplus
}
#endif
#endif /* ZRC4_H */
