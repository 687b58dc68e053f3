/*
 * include/curve25519_amd.h -- batched entry points of the MI355X engine (C ABI).
 *
 * The reference has no batch API: its callers loop over the single-call functions of
 * include/curve25519_dh.h and include/ed25519_signature.h (e.g. test/curve25519_test.c:144-318).
 * Each function below is the N-element form of exactly one reference call and produces, element by
 * element, the bytes that call would produce.  Layouts are contiguous fixed-stride arrays:
 *
 *     sk, pk, shared : n x 32 bytes          priv, sig : n x 64 bytes
 *     msg            : n x msg_size bytes    verdict   : n x int (1 valid / 0 invalid)
 *
 * Two flavours:
 *   *_batch : host pointers.  Synchronous: uploads, runs the kernels, downloads.  Callable from
 *             several host threads at once (each thread owns its stream and staging buffers).
 *   *_dev   : device pointers (hipMalloc'ed memory of the current device, 16-byte aligned) and a
 *             hipStream_t passed as void* (NULL = default stream).  Asynchronous: returns after
 *             enqueueing.  This is what bench.py times with inputs resident in HBM.
 *
 * Return value: 0 on success, otherwise a HIP error code (c25519_amd_last_error() gives the text).
 * There is no CPU fallback: without a usable gfx950 device every entry point fails.
 */
#ifndef CURVE25519_AMD_H
#define CURVE25519_AMD_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* library / device status ------------------------------------------------------------------- */
const char *c25519_amd_version(void);
const char *c25519_amd_last_error(void);               /* per-thread: the text of the last call of this thread, "" if it succeeded */
int  c25519_amd_device_count(void);                    /* usable HIP devices (0 when none) */
int  c25519_amd_set_device(int device);                /* device used by this host thread */
/* Tuning / A-B knobs.  Each knob is read ONCE from the environment variable C25519_AMD_<name> when the library is first
 * used (no getenv() on any call path afterwards) and can be changed at run time here; value < 0 restores the built-in
 * choice.  Names: COOP_MAX (largest batch that runs one operation per wave; 0 = never), XF_SPLIT (X25519 as two launches 1 /
 * one fused launch 0), INV_K (elements per inverting lane, 1..16), VERIFY_REFERENCE_ORDER (1: every verification in the
 * reference's 4-fold + 8-fold order), MULTI_FORCE_GATHER (1: a one-device *_multi handle gathers too), MULTI_VIRTUAL (V: a
 * one-device list given to c25519_amd_multi_create becomes V virtual devices on it), BASE_COMB (fixed-base walks: 0 = the 8 x 32 comb staged in LDS,
 * 1 = the wide 13 x 20 comb read through L2, the default), HELPER_THREADS (cap on the staging helper threads; default: the CPUs this process may use),
 * VERIFY_LAT_CAP_BITS (test knob, 100..157: verification's lattice walk refuses longer short vectors, which then take the
 * reference-order kernel), ONE_KEY_WIDE (ed25519_Verify_Check_*: the smallest batch that BUILDS a wide comb for its one key,
 * default 65536; a call of more than 1024 pairs whose context is the one the calling thread's last such batch built a comb for
 * walks that comb whatever its size; 0 = never), LADDER2_MAX (curve25519_dh_CreateSharedKey_*: the largest call that runs the
 * ladder on two waves per element, default 512; 0 = never), QUAD_MIN / QUAD_MAX (calls of more than QUAD_MIN and at most QUAD_MAX
 * elements run FOUR LANES per element -- X25519: the whole operation, defaults 3584 / 32768; ed25519_VerifySignature_*: scalars
 * and point tables side by side, the walk on quads, defaults 1024 / 32768; key pairs, signatures, CalculatePublicKey_fast and the
 * one-key ed25519_Verify_Check_* with a comb: the whole operation in one launch, defaults 1024 / 16384; QUAD_MAX = 0: never),
 * ONE_PEER_WIDE (curve25519_dh_CreateSharedKey_one_peer_*: the smallest batch that BUILDS a wide comb for a new peer key; a call
 * of more than 3584 elements with the peer the calling thread's last comb was built for walks that comb whatever its size;
 * default 98304; 0 = never), PEER_INDEXED_MIN (curve25519_dh_CreateSharedKey_indexed_*: the smallest batch that walks the peer
 * contexts' rows; smaller calls gather the contexts' keys and run what curve25519_dh_CreateSharedKey_dev runs; default 2049;
 * 0 = always walk), BATCH_EQ_MIN / BATCH_EQ_WINDOW / BATCH_EQ_INDEXED_MIN (ed25519_VerifyBatch_zip215_*, see there), SCALARMULT_WINDOW
 * (ed25519_ScalarMult_* and ristretto255_ScalarMult_*: the window width of the variable-base walk, 2, 3 or 4; anything else: the built-in choice, 2, the fastest at 2^20),
 * SC_INVERT_K (ed25519_ScalarInvert_*: elements per inverting lane, 1, 2, 4, 8 or 16; anything else: the built-in choice by n, see there),
 * MSM_BUCKET_MIN / MSM_WINDOW (*_MultiScalarMult_vartime_*, see there).
 * _get returns -1 for "built-in choice", -2 for an unknown name.
 * Environment only (read once): C25519_AMD_DONE_WORD=0 -- a host-pointer call of ONE element waits for the stream's event instead of
 * the completion word its last kernel stores behind the results (5 us later; same bytes); C25519_AMD_ZERO_COPY=0 -- calls of a
 * few elements are staged through device buffers like any batch. */
int  c25519_amd_tunable_set(const char *name, long value);
long c25519_amd_tunable_get(const char *name);
int  c25519_amd_usable_cpus(void);                     /* CPUs this process may use (affinity mask cut to the cgroup quota) */
/* *_dev calls a thread issues on different streams may overlap on the device: each stream gets its own work scratch (up
 * to four per device; a further stream reuses the least recently used one after waiting for it).  Splitting a mixed batch
 * over streams is worth ~13 % (one operation's last round of workgroups fills up with the next operation's).
 * Each host thread that calls into the library owns four streams, eight sets of pinned + device staging buffers and work
 * scratch slabs, all on the device that was current at its first call (they follow the thread to another device on
 * the next call, released on the old one first).  They are freed when the thread exits; a long-lived thread can
 * give them back earlier with this call.  Staging buffers are zeroed before they are freed.
 * Process exit: exit() may be called while other threads are inside library calls -- the library's atexit handler lets the
 * calls in flight finish (it waits up to 10 s) before the HIP runtime is torn down, a thread that calls again afterwards is
 * parked for the rest of the process' life, and a call made by the exiting thread itself (from a static destructor or an
 * atexit handler of the caller's) returns hipErrorDeinitialized (release / destroy calls: return at once). */
void c25519_amd_thread_release(void);

/* Optional: page-lock a host array the caller is going to pass to *_batch functions again and again (hipHostRegister).
 * A *_batch call recognises page-locked arguments (registered here, or allocated with hipHostMalloc) and lets the DMA
 * engines read / write them directly instead of staging them through its own pinned buffers: no CPU copy at all.
 * Registration costs about a millisecond per 100 MB: worth it for buffers that are reused.  Unregister before free().
 * Page locking works on whole pages, so p must be 4 KiB-aligned and bytes a multiple of 4 KiB (posix_memalign / mmap a
 * buffer of its own: a heap object that shares a page with a neighbour would lock and unlock the neighbour with it);
 * anything else is refused. */
int c25519_amd_host_register(void *p, size_t bytes);
int c25519_amd_host_unregister(void *p);

/* X25519 ------------------------------------------------------------------------------------ */
/* n x curve25519_dh_CreateSharedKey (reference include/curve25519_dh.h:45); sk is clamped in place */
int curve25519_dh_CreateSharedKey_batch(unsigned char *shared, const unsigned char *pk,
                                        unsigned char *sk, size_t n);
int curve25519_dh_CreateSharedKey_dev(void *shared, const void *pk, void *sk, size_t n, void *stream);

/* n x curve25519_dh_CreateSharedKey with the SAME 32-byte peer key pk for every element (sealed-box / HPKE-style encryption of
 * many records to one recipient, a server re-keying many ephemeral secrets against one static key); sk is clamped in place.
 * Byte-identical to curve25519_dh_CreateSharedKey_* with pk repeated n times, for every pk.  From ONE_PEER_WIDE elements per
 * call (tunable, see above) a peer on the curve gets a wide fixed-base comb built for 8 * pk (0.6 ms; kept in 2 MiB of device
 * memory per calling thread until the thread exits or calls c25519_amd_thread_release()), and the call walks it instead of
 * the Montgomery ladder; a later call of more than the per-wave sizes (3584 elements) with the same pk walks the kept comb
 * whatever its size.  Other calls, and peers on the twist (or u = -1), run the ladder.  The _dev form does not synchronise: pk is read on
 * the device. */
int curve25519_dh_CreateSharedKey_one_peer_batch(unsigned char *shared, const unsigned char *pk /* 32 bytes */,
                                                 unsigned char *sk, size_t n);
int curve25519_dh_CreateSharedKey_one_peer_dev(void *shared, const void *pk /* 32 bytes, device */, void *sk, size_t n,
                                               void *stream);
/* did the calling thread's last curve25519_dh_CreateSharedKey_one_peer_* call on this device walk the peer's comb (1) or the
 * ladder (0)?  -1: no such call.  Synchronises with that call's stream.  (A *_batch call of several pieces reports its last piece.) */
long c25519_amd_x25519_one_peer_last_wide(void);

/* X25519 against MANY peer keys in one call: a mixed stream of secrets, each against one of n_ctx known peers (static-static DH
 * with configured peers, records sealed to many recipients).  A peer context is C25519_AMD_PEER_CTX_SIZE bytes, deterministic
 * (the same key always gives the same bytes) and free of pointers (it may be copied or stored):
 *   bytes 0..31     the peer key exactly as given (the ladder reads it)
 *   bytes 32..35    uint32 eligibility: 1 = the rows stand in for the ladder, 0 = the ladder decides
 *   bytes 36..63    zero
 *   bytes 64..1599  16 rows of 96 bytes.  Row k = sum over the set bits i of k of 2^(64 i) * Q, Q = 8 * P, P the point of u = the
 *                   key read as 256 bits mod p (x the root ed25519's decoding picks for parity 0), affine (Z = 1), stored as
 *                   Y+X | Y-X | 2d*X*Y, three field elements of eight canonical little-endian 32-bit words.  Row 0 is (1, 1, 0).
 *                   A small-order P has 16 neutral rows (its shared keys are 0, as from the ladder).  A key on the twist, and
 *                   u = -1, have eligibility 0 and zero rows.
 * A context is trusted data, like a key store: a modified context gives an unspecified output, and since its rows need not lie
 * in the curve's prime-order subgroup, it can reveal bits of the secret to whoever chose them.  It still reads nothing outside
 * ctxs.  The index is public data: its gather is not constant-time; the secret only selects rows.
 * curve25519_dh_CreateSharedKey_indexed_*: n x curve25519_dh_CreateSharedKey(shared_i, ctxs[ctx_index[i]].pk, sk_i), sk clamped
 * in place; every output byte and clamped sk byte equals what curve25519_dh_CreateSharedKey_* gives for the key in the element's
 * context.  ctx_index is n x uint32.
 *   n == 0 returns 0; a null pointer, or n_ctx == 0 with n > 0, is an argument error.
 *   *_batch checks every index on the host: one >= n_ctx refuses the call before any work, shared and sk untouched.  It uploads
 *   the contexts once per call into a device buffer of the calling thread (grow-only; zeroed before it is freed by
 *   c25519_amd_thread_release() or a larger call).
 *   *_dev never synchronises: an index >= n_ctx is a context for the key 0 (32 zero bytes, sk still clamped) and nothing outside
 *   ctxs is read.
 * From PEER_INDEXED_MIN elements per call (tunable, see above) each element walks its own context's rows in place (64 doublings
 * and 64 mixed additions); elements of ineligible contexts run the ladder in a second kernel.  Smaller calls gather the keys and
 * run what curve25519_dh_CreateSharedKey_dev runs at their size (profiles/peer_indexed_rate.txt). */
#define C25519_AMD_PEER_CTX_SIZE 1600
int curve25519_dh_Peer_Init_batch(void *ctx, const unsigned char *pk, size_t n);          /* n x 1600 bytes */
int curve25519_dh_Peer_Init_dev(void *ctx, const void *pk, size_t n, void *stream);
int curve25519_dh_CreateSharedKey_indexed_batch(unsigned char *shared, const void *ctxs, size_t n_ctx,
                                                const uint32_t *ctx_index, unsigned char *sk, size_t n);
int curve25519_dh_CreateSharedKey_indexed_dev(void *shared, const void *ctxs, size_t n_ctx, const void *ctx_index,
                                              void *sk, size_t n, void *stream);
/* how many elements of the calling thread's last curve25519_dh_CreateSharedKey_indexed_* call on this device ran the ladder (all of
 * them below PEER_INDEXED_MIN, else those of ineligible contexts)?  -1: no such call.  Synchronises with that call's stream.  (A
 * *_batch call of several pieces reports its last piece.) */
long c25519_amd_x25519_indexed_last_ladder_elements(void);

/* n x curve25519_dh_CalculatePublicKey (reference :34): ladder on the base point u = 9 */
int curve25519_dh_CalculatePublicKey_batch(unsigned char *pk, unsigned char *sk, size_t n);
int curve25519_dh_CalculatePublicKey_dev(void *pk, void *sk, size_t n, void *stream);

/* n x curve25519_dh_CalculatePublicKey_fast (reference :40): Edwards 8-fold walk + birational map */
int curve25519_dh_CalculatePublicKey_fast_batch(unsigned char *pk, unsigned char *sk, size_t n);
int curve25519_dh_CalculatePublicKey_fast_dev(void *pk, void *sk, size_t n, void *stream);

/* Ed25519 ----------------------------------------------------------------------------------- */
/* n x ed25519_CreateKeyPair (reference include/ed25519_signature.h:40), blinding = NULL */
int ed25519_CreateKeyPair_batch(unsigned char *pub, unsigned char *priv, const unsigned char *sk, size_t n);
int ed25519_CreateKeyPair_dev(void *pub, void *priv, const void *sk, size_t n, void *stream);

/* n x ed25519_SignMessage (reference :47), blinding = NULL, all messages msg_size bytes long */
int ed25519_SignMessage_batch(unsigned char *sig, const unsigned char *priv, const unsigned char *msg,
                              size_t msg_size, size_t n);
int ed25519_SignMessage_dev(void *sig, const void *priv, const void *msg, size_t msg_size, size_t n,
                            void *stream);

/* Blinding (reference include/ed25519_signature.h:54-64, source/ed25519_sign.c:246-331).  A context is 192 bytes --
 * the reference's EDP_BLINDING_CTX size: scalar bl = L - t, 32 random bytes zr, and t*B as four canonical 32-byte
 * elements.  ed25519_Blinding_Init (declared in ed25519_signature.h) derives it ON THE DEVICE from the caller's seed;
 * the functions below take ONE context for the whole batch and compute (k + bl)*B + BP from a Z-randomised starting
 * point, so the walk and its secret-indexed table lookups see a different scalar under every context.  Outputs are
 * byte-identical to the unblinded calls (as in the reference). */
int ed25519_Blinding_Init_dev(void *ctx /* 192 bytes */, const void *seed, size_t seed_len, void *stream);
int ed25519_CreateKeyPair_blinded_batch(unsigned char *pub, unsigned char *priv, const void *blinding,
                                        const unsigned char *sk, size_t n);
int ed25519_CreateKeyPair_blinded_dev(void *pub, void *priv, const void *blinding, const void *sk, size_t n,
                                      void *stream);
int ed25519_SignMessage_blinded_batch(unsigned char *sig, const unsigned char *priv, const void *blinding,
                                      const unsigned char *msg, size_t msg_size, size_t n);
int ed25519_SignMessage_blinded_dev(void *sig, const void *priv, const void *blinding, const void *msg,
                                    size_t msg_size, size_t n, void *stream);

/* the same with messages of different lengths: message i is msgs[offsets[i] .. offsets[i+1]),
 * offsets has n+1 entries (host memory for _batch, device memory for _dev) */
int ed25519_SignMessage_ragged_batch(unsigned char *sig, const unsigned char *priv, const unsigned char *msgs,
                                     const uint64_t *offsets, size_t n);
int ed25519_SignMessage_ragged_dev(void *sig, const void *priv, const void *msgs, const uint64_t *offsets,
                                   size_t n, void *stream);

/* Signing under MANY keys in one call: a mixed stream of messages, each naming one of n_ctx signer contexts (a signing service
 * with a key store).  A signer context is C25519_AMD_SIGN_CTX_SIZE bytes, built by ed25519_Sign_Init_* from the 64-byte privKey
 * (seed || pk); deterministic and free of pointers:
 *   bytes 0..31     a = SHA-512(seed)[0..31] after ecp_TrimSecretKey (the clamped scalar), little-endian
 *   bytes 32..63    prefix = SHA-512(seed)[32..63]
 *   bytes 64..95    pk = privKey[32..63] as given (not recomputed: the reference hashes the given half)
 *   bytes 96..127   zero
 * A context is as secret as the private key it came from.  A context with other bytes is still defined: element i's signature
 * is R = r*B, S = (h*a + r) mod L with r = H(prefix || m) mod L and h = H(enc(R) || pk || m), using the context's a (any
 * 256-bit value), prefix and pk; bytes 96..127 are ignored.  The index is public data: its gather is not constant-time; the
 * secret only enters the hashes and the comb walk, as in ed25519_SignMessage_*.
 * ed25519_SignMessage_indexed_*: signature i is byte-identical to ed25519_SignMessage_*(priv[ctx_index[i]], m_i) when the contexts
 * came from ed25519_Sign_Init_* on priv -- for every priv, one whose pk half is not its seed's included.  ctx_index is n x uint32.
 *   n == 0 returns 0; a null pointer, or n_ctx == 0 with n > 0, is an argument error.
 *   *_batch checks every index on the host: one >= n_ctx refuses the call before any work, sig untouched.  It uploads the
 *   contexts once per call into a device buffer of the calling thread (grow-only; zeroed before it is freed by
 *   c25519_amd_thread_release() or a larger call).
 *   *_dev never synchronises: an index >= n_ctx gives 64 zero bytes and nothing outside ctxs is read.
 * The calls run the forms ed25519_SignMessage_dev runs at their size (the same tunables) without the per-signature SHA-512 of
 * the seed; a context is never carried in kernel arguments (profiles/sign_indexed_rate.txt). */
#define C25519_AMD_SIGN_CTX_SIZE 128
int ed25519_Sign_Init_batch(void *ctx, const unsigned char *priv, size_t n);          /* n x 64 -> n x 128 bytes */
int ed25519_Sign_Init_dev(void *ctx, const void *priv, size_t n, void *stream);
int ed25519_SignMessage_indexed_batch(unsigned char *sig, const void *ctxs, size_t n_ctx, const uint32_t *ctx_index,
                                      const unsigned char *msg, size_t msg_size, size_t n);
int ed25519_SignMessage_indexed_dev(void *sig, const void *ctxs, size_t n_ctx, const void *ctx_index,
                                    const void *msg, size_t msg_size, size_t n, void *stream);
int ed25519_SignMessage_indexed_ragged_batch(unsigned char *sig, const void *ctxs, size_t n_ctx, const uint32_t *ctx_index,
                                             const unsigned char *msgs, const uint64_t *offsets, size_t n);
int ed25519_SignMessage_indexed_ragged_dev(void *sig, const void *ctxs, size_t n_ctx, const void *ctx_index,
                                           const void *msgs, const uint64_t *offsets, size_t n, void *stream);

/* Key classification, and conversion of an Ed25519 identity to the X25519 key of the same secret.
 * ed25519_ClassifyKey_*: flags[i] is the OR of the bits below for the 32 key bytes pk[i].  Read y = the low 255 bits as a
 * little-endian integer and sign = bit 255; p = 2^255 - 19, L the order of the base point, O the neutral element (0, 1).
 *   DECODES       the bytes decode as the ZIP-215 calls decode a key: y is taken mod p (all of [p, 2^255) accepted) and
 *                 (y^2 - 1) / (d y^2 + 1) has a square root x; the root with parity sign is A's x, and x = 0 whatever sign says.
 *   CANONICAL     y < p, and not (the decoded x is 0 with sign = 1); for bytes that do not decode: y < p.
 *   SMALL_ORDER   the bytes decode and [8]A = O (y mod p is one of 0, 1, p - 1, y8, p - y8, y8 the y of a point of order 8).
 *   TORSION_FREE  the bytes decode and [L]A = O: A lies in the subgroup of prime order.  O itself has both order bits.
 * Bits 2 and 3 are clear where bit 0 is.  dalek's is_torsion_free is bit 3, is_small_order bit 2; a key passes libsodium's
 * crypto_core_ed25519_is_valid_point exactly when flags == 11 (canonical, on the curve, not of small order, in the prime-order
 * subgroup).  That is libsodium's rule as stated here: the stated rule is the contract, the library was not compared with a
 * libsodium build.  A mixed-order key a*B + T (T of order 2, 4 or 8) has flags 3: it decodes, is canonical and is not of small
 * order, and only the walk [L]A tells it from an honest key -- which is what a caller who must bound verification latency, or who
 * will not accept such keys, screens with.
 * ed25519_PublicKey_to_X25519_*: libsodium's crypto_sign_ed25519_pk_to_curve25519.  ok[i] = 1 exactly when the key decodes, is not
 * of small order and is torsion-free, (flags & 13) == 9; a canonical encoding is not required.  xpk[i] is then the canonical 32
 * bytes of u = (1 + y) / (1 - y) mod p, bit 255 clear; otherwise ok[i] = 0 and xpk[i] is 32 zero bytes.  Every row of xpk and ok is
 * written.  The result is curve25519_dh_CalculatePublicKey of ed25519_PrivateKey_to_X25519's output for the same key pair, so it
 * can go through curve25519_dh_Peer_Init_* into curve25519_dh_CreateSharedKey_indexed_* (INTEGRATION.md).
 * ed25519_PrivateKey_to_X25519_*: libsodium's crypto_sign_ed25519_sk_to_curve25519.  priv is n x 64 bytes, the reference's
 * privKey (seed || public key): xsk[i] = SHA-512(priv[i][0..31])[0..31] with xsk[i][0] &= 248, xsk[i][31] &= 127, xsk[i][31] |= 64;
 * bytes 32..63 of priv are ignored.  xsk is as secret as the seed: one SHA-512 compression per element, no branch and no address
 * that depends on the data (what ed25519_Sign_Init_* puts in bytes 0..31 of a signer context).
 *   n == 0 returns 0; a null pointer is an argument error.  *_dev forms never synchronise and take 16-byte aligned device
 *   pointers (flags and ok: n x 4 bytes); *_batch forms stage through the calling thread's pipeline like their neighbours.
 * One lane per key at every n (no per-wave or four-lane form; c25519_amd_last_shape is not written).  The lane's work is the walk
 * [L]A by the signed non-adjacent form of L: 252 doublings and 45 mixed additions, about 2,100 field products per key, and a call
 * of a few keys costs one lane's latency of that walk.  Measured (profiles/key_convert_rate.txt): up to 2^16 keys a call takes
 * 0.58-0.64 ms whatever its size, a call of ONE key 0.59-0.68 ms (ClassifyKey_dev) / 0.62-0.73 ms (PublicKey_to_X25519_dev), where
 * ed25519_VerifySignature_dev takes 0.13 ms; at 2^20 ClassifyKey_dev runs 125 M keys/s and PublicKey_to_X25519_dev 129 M/s, 1.11 x and
 * 1.14 x ed25519_VerifySignature_dev of the same build (2^16: 1.18 x / 1.14 x; 2^14: 0.57 x / 0.55 x; 2^10: 0.50 x / 0.48 x);
 * PrivateKey_to_X25519_dev 10.6 G keys/s at 2^20, 23 us for one key.  Convert a key set once, like Peer_Init, not per record. */
#define C25519_AMD_KEY_DECODES      1u
#define C25519_AMD_KEY_CANONICAL    2u
#define C25519_AMD_KEY_SMALL_ORDER  4u
#define C25519_AMD_KEY_TORSION_FREE 8u
int ed25519_ClassifyKey_batch(uint32_t *flags, const unsigned char *pk, size_t n);
int ed25519_ClassifyKey_dev(void *flags, const void *pk, size_t n, void *stream);
int ed25519_PublicKey_to_X25519_batch(unsigned char *xpk, int *ok, const unsigned char *pk, size_t n);
int ed25519_PublicKey_to_X25519_dev(void *xpk, void *ok, const void *pk, size_t n, void *stream);
int ed25519_PrivateKey_to_X25519_batch(unsigned char *xsk, const unsigned char *priv /* n x 64 */, size_t n);
int ed25519_PrivateKey_to_X25519_dev(void *xsk, const void *priv, size_t n, void *stream);

/* Group operations on Ed25519 points: libsodium's crypto_scalarmult_ed25519[_noclamp], crypto_scalarmult_ed25519_base[_noclamp] and
 * crypto_core_ed25519_add / _sub, dalek's EdwardsPoint * Scalar -- what key blinding, hierarchical child keys (A + [z]B), threshold
 * and adaptor signatures and Diffie-Hellman on Edwards keys are built from.  Points and scalars are n x 32 bytes, ok is n x int.
 *   Decoding.  A point decodes exactly as ed25519_ClassifyKey_*'s DECODES bit says: the ZIP-215 rule, y = the low 255 bits taken
 *     mod p, x the square root of (y^2 - 1) / (d y^2 + 1) with the parity of bit 255, and x = 0 whatever that bit says.
 *   Scalar.  e is the 32-byte scalar clamped on a COPY (byte 0 &= 248, byte 31 &= 127, byte 31 |= 64); for the _noclamp calls e is the
 *     low 255 bits: bit 255 is ignored, as libsodium ignores it.  The caller's scalar bytes are never written (the X25519 calls
 *     clamp theirs in place; these do not).
 *   ed25519_ScalarMult[_noclamp]_*: ok[i] = 1 exactly when point[i] decodes, and q[i] is then the canonical encoding of [e]P: y < p
 *     little-endian, bit 255 the parity of x, clear for x = 0; the neutral element is 01 00 .. 00 with ok = 1.  Otherwise ok[i] = 0
 *     and q[i] is 32 zero bytes.  Every row of q and ok is written.  No rule on the point's order and none on canonical input is
 *     applied.  libsodium's call returns 0 with the same bytes exactly when ed25519_ClassifyKey_* gives flags == 11 for the point and
 *     q is not the neutral encoding; that is libsodium's rule as stated here: the stated rule is the contract, the library was not
 *     compared with a libsodium build.  A _noclamp result on a mixed-order point reveals the scalar mod 8 (the clamped calls multiply
 *     by a multiple of 8); ed25519_ClassifyKey_* screens for such points.
 *   ed25519_ScalarMultBase[_noclamp]_*: q[i] = enc([e]B) for every 32-byte scalar (e = 0 gives the neutral encoding).
 *   ed25519_PointAdd_* / ed25519_PointSub_*: ok[i] = 1 exactly when p[i] and q[i] both decode, and then r[i] = enc(P + Q) / enc(P - Q);
 *     otherwise r[i] is 32 zero bytes and ok[i] = 0.
 *   Secrecy.  The scalar is secret, points are public.  In ed25519_ScalarMult* no branch condition and no load or store address
 *     derives from the scalar, not even a row fetch: the walk keeps its table of multiples of P in registers and selects a row by
 *     masks over all of them.  ed25519_ScalarMultBase* fetches the base comb's rows by secret index, exactly as key pairs and signing
 *     do.
 *   n == 0 returns 0; a null pointer is an argument error.  *_dev forms never synchronise and take 16-byte aligned device
 *   pointers; *_batch forms stage through the calling thread's pipeline like their neighbours.
 * One lane per element at every n (no per-wave or four-lane form; c25519_amd_last_shape is not written), so a call of a few
 * elements costs one lane's latency of the walk.  ed25519_ScalarMult* recodes e into signed W-bit digits and walks 129 / 86 / 65 of
 * them for W = 2 / 3 / 4 (tunable SCALARMULT_WINDOW), about 2,840 / 2,520 / 2,400 field products per element against the X25519
 * ladder's 2,550.  Measured (profiles/group_ops_rate.txt, interleaved rounds): at 2^20 ScalarMult_dev runs 90.4 M/s at W = 2 (11.60 ms),
 * 86.3 at W = 3, 87.5 at W = 4, against 130.8 M/s for curve25519_dh_CreateSharedKey_dev of the same build on the same n: 0.69 x /
 * 0.66 x / 0.67 x the ladder, not the 0.85-1.15 x the counts had suggested (the walk holds two waves per SIMD at W = 2 and one at
 * W = 3 and 4, the ladder four).  W = 2 wins by 0.39 ms where the rounds spread over 0.07 ms, so it is the built-in width.  Up to 2^16
 * elements a call is one lane's latency of the walk, 0.85-0.86 ms at W = 2 (0.78 at W = 3, 0.76-0.78 at W = 4: the wider windows are
 * the shorter walks where latency counts), a call of ONE element 0.86-1.02 ms; the _noclamp calls cost the same.
 * ScalarMultBase_dev: 1.29-1.31 G/s at 2^20, 0.08-0.09 ms up to 2^16, one element 86-96 us.  PointAdd_dev / PointSub_dev: 658-667 M/s
 * at 2^20, 0.15 ms up to 2^16, one element 0.15-0.17 ms. */
int ed25519_ScalarMult_batch(unsigned char *q, int *ok, const unsigned char *scalar, const unsigned char *point, size_t n);
int ed25519_ScalarMult_dev(void *q, void *ok, const void *scalar, const void *point, size_t n, void *stream);
int ed25519_ScalarMult_noclamp_batch(unsigned char *q, int *ok, const unsigned char *scalar, const unsigned char *point, size_t n);
int ed25519_ScalarMult_noclamp_dev(void *q, void *ok, const void *scalar, const void *point, size_t n, void *stream);
int ed25519_ScalarMultBase_batch(unsigned char *q, const unsigned char *scalar, size_t n);
int ed25519_ScalarMultBase_dev(void *q, const void *scalar, size_t n, void *stream);
int ed25519_ScalarMultBase_noclamp_batch(unsigned char *q, const unsigned char *scalar, size_t n);
int ed25519_ScalarMultBase_noclamp_dev(void *q, const void *scalar, size_t n, void *stream);
int ed25519_PointAdd_batch(unsigned char *r, int *ok, const unsigned char *p, const unsigned char *q, size_t n);
int ed25519_PointAdd_dev(void *r, void *ok, const void *p, const void *q, size_t n, void *stream);
int ed25519_PointSub_batch(unsigned char *r, int *ok, const unsigned char *p, const unsigned char *q, size_t n);
int ed25519_PointSub_dev(void *r, void *ok, const void *p, const void *q, size_t n, void *stream);

/* ristretto255 (RFC 9496): the prime-order group built on the same curve -- libsodium's crypto_core_ristretto255_* and
 * crypto_scalarmult_ristretto255[_base], dalek's RistrettoPoint -- for OPRF / private set intersection, VOPRF and Privacy Pass
 * issuance, Pedersen and Bulletproofs generators, Schnorrkel.  An element is 32 bytes; there is no cofactor, so no point has to be
 * screened before it meets a secret scalar and no result reveals the scalar mod 8 (the _noclamp Edwards calls above need
 * ed25519_ClassifyKey_* for that, a second walk as long as the multiplication).  Elements and scalars are n x 32 bytes, hash is
 * n x 64 bytes, ok is n x int.
 *   Decoding.  32 bytes decode exactly when DECODE of RFC 9496 section 4.3.1 succeeds: s < p, s even, the square root exists, t is
 *     non-negative and y != 0.  There is no Edwards y / sign-bit form; the encodings the Edwards calls take are not ristretto255's.
 *   ristretto255_IsValidPoint_*: ok[i] = 1 exactly when point[i] decodes, else 0 (crypto_core_ristretto255_is_valid_point).
 *   ristretto255_FromHash_*: p[i] = ENCODE(MAP(low half) + MAP(high half)) of section 4.3.4 for the 64 bytes hash[i]: each half is
 *     read little-endian with bit 255 masked and taken mod p (crypto_core_ristretto255_from_hash, dalek's from_uniform_bytes).  It
 *     cannot fail: there is no ok array.
 *   Scalar.  e is the low 255 bits of the 32-byte scalar: no clamp, bit 255 ignored as in the _noclamp Edwards calls.  The caller's
 *     scalar bytes are never written.
 *   ristretto255_ScalarMult_*: ok[i] = 1 exactly when point[i] decodes, and then q[i] = ENCODE([e]P); the identity encodes as 32 zero
 *     bytes with ok = 1.  Otherwise ok[i] = 0 and q[i] is 32 zero bytes.  libsodium's crypto_scalarmult_ristretto255 additionally
 *     returns -1 for an identity result; this call gives ok = 1 and the zero bytes (compare q with zero where that matters).
 *   ristretto255_ScalarMultBase_*: q[i] = ENCODE([e]B) for every 32-byte scalar, over the wide comb (e = 0 mod L gives zero bytes;
 *     libsodium's _base returns -1 there).
 *   ristretto255_PointAdd_* / ristretto255_PointSub_*: ok[i] = 1 exactly when p[i] and q[i] both decode, and then
 *     r[i] = ENCODE(P + Q) / ENCODE(P - Q); otherwise r[i] is 32 zero bytes and ok[i] = 0.
 *   Every row of every output is written.  n == 0 returns 0; a null pointer is an argument error.  *_dev forms never synchronise
 *   and take 16-byte aligned device pointers; *_batch forms stage through the calling thread's pipeline like their neighbours.
 *   Secrecy.  The scalar and the 64 hash bytes are secret; point encodings are public.  No branch condition and no load or store
 *     address derives from the scalar in ristretto255_ScalarMult_* (decoding and encoding included) or from the hash bytes in
 *     ristretto255_FromHash_*: every comparison of the square-root step, the rotation and the negations of the encoding and the
 *     selections of the map are masks.  ristretto255_ScalarMultBase_* fetches the base comb's rows by secret index, exactly as
 *     ed25519_ScalarMultBase_*, key pairs and signing do.
 * One lane per element at every n (no per-wave or four-lane form; c25519_amd_last_shape is not written) and ONE kernel per call: the
 * encoding's inverse square root cannot be shared between elements as an inversion can, so it runs in the lane (one x^((p-5)/8)
 * chain, 254 squarings and 11 products) and no call leases scratch.  The walk's and the comb's last additions do not form T, which
 * the encoding reads: the point is re-formed as (X Z, Y Z, Z^2, X Y) in front of it (three products and a squaring), and the walk
 * stays as the Edwards calls run it.  ristretto255_ScalarMult_* is decode, the Edwards calls' variable-base walk (tunable
 * SCALARMULT_WINDOW: W = 2, 3 or 4) and encode in one kernel: the walk's products plus two chains.  FromHash is three chains,
 * ScalarMultBase the comb plus one chain, PointAdd / PointSub three chains, IsValidPoint one.
 * Measured (profiles/ristretto_rate.txt, interleaved rounds, the Edwards call of the same build on the same n beside each): at 2^20
 * ScalarMult_dev runs 86.2 M/s at W = 2 (12.16 ms), 82.5 at W = 3, 80.7 at W = 4, against 91.9 / 86.0 / 87.3 M/s for
 * ed25519_ScalarMult_noclamp_dev: 0.94 x / 0.96 x / 0.93 x.  The counts said so: a chain measures 0.75-0.80 ms per 2^20 elements
 * (IsValidPoint_dev, one chain and a dozen products: 0.77 ms, 1.36 G/s), the Edwards call already pays one for its own decoding, and
 * the second chain with the re-formed point replaces that call's share of the batch inversion.  W = 2 wins by 0.55 ms where the rounds
 * spread over 0.02 ms and is the built-in width, as for the Edwards calls.  ScalarMultBase_dev: 680 M/s (1.54 ms) against 1.31 G/s for
 * ed25519_ScalarMultBase_noclamp_dev, 0.52 x: the chain is half of the call, as expected.  PointAdd_dev / PointSub_dev: 437-445 M/s
 * (2.36-2.40 ms, 0.67-0.68 x ed25519_PointAdd_dev's 656 M/s); FromHash_dev: 434 M/s (2.41 ms, three chains).  Up to 2^16 elements a
 * call is one lane's latency: 0.88-0.89 ms for ScalarMult at W = 2 (0.79-0.80 at W = 3), 0.12-0.13 ms for ScalarMultBase, 0.19-0.20 ms
 * for PointAdd / PointSub / FromHash, 0.07 ms for IsValidPoint; a call of ONE element 0.88-1.02 ms / 0.13-0.15 / 0.19-0.22 / 0.07-0.08 ms. */
int ristretto255_IsValidPoint_batch(int *ok, const unsigned char *point, size_t n);
int ristretto255_IsValidPoint_dev(void *ok, const void *point, size_t n, void *stream);
int ristretto255_FromHash_batch(unsigned char *p, const unsigned char *hash /* n x 64 */, size_t n);
int ristretto255_FromHash_dev(void *p, const void *hash, size_t n, void *stream);
int ristretto255_ScalarMult_batch(unsigned char *q, int *ok, const unsigned char *scalar, const unsigned char *point, size_t n);
int ristretto255_ScalarMult_dev(void *q, void *ok, const void *scalar, const void *point, size_t n, void *stream);
int ristretto255_ScalarMultBase_batch(unsigned char *q, const unsigned char *scalar, size_t n);
int ristretto255_ScalarMultBase_dev(void *q, const void *scalar, size_t n, void *stream);
int ristretto255_PointAdd_batch(unsigned char *r, int *ok, const unsigned char *p, const unsigned char *q, size_t n);
int ristretto255_PointAdd_dev(void *r, void *ok, const void *p, const void *q, size_t n, void *stream);
int ristretto255_PointSub_batch(unsigned char *r, int *ok, const unsigned char *p, const unsigned char *q, size_t n);
int ristretto255_PointSub_dev(void *r, void *ok, const void *p, const void *q, size_t n, void *stream);

/* The scalar field: arithmetic mod L = 2^252 + 27742317777372353535851937790883648493, the order of the base point -- libsodium's
 * crypto_core_ed25519_scalar_* and crypto_core_ristretto255_scalar_* (the same functions under two names there, ONE set of names
 * here), ref10's sc25519_muladd, dalek's Scalar -- so that a protocol over the group calls above stays on the device: an OPRF
 * evaluation is unblinded by 1/r, a Schnorr or DLEQ response is k + c x, a hash becomes a scalar by a 64-byte reduction.
 * A scalar is 32 little-endian bytes per element (ScalarReduce's input: 64); ok is n x int.
 *   Inputs.  Every input may be ANY 32-byte value, not only a reduced one: it stands for its value mod L.  (libsodium asks for
 *     reduced inputs in _scalar_mul; there is no such condition here.)
 *   Outputs.  Every output is the canonical representative in [0, L).
 *   ed25519_ScalarReduce_*: r[i] = s[i] mod L for the 512-bit s[i] (_scalar_reduce).
 *   ed25519_ScalarAdd_* / _ScalarSub_* / _ScalarMul_*: z[i] = x[i] + y[i] / x[i] - y[i] / x[i] y[i] (_scalar_add / _sub / _mul).
 *   ed25519_ScalarNegate_*: r[i] = -s[i] (_scalar_negate).  ed25519_ScalarComplement_*: r[i] = 1 - s[i] (_scalar_complement).
 *   ed25519_ScalarMulAdd_*: r[i] = a[i] b[i] + c[i] (sc25519_muladd).
 *   ed25519_ScalarInvert_*: ok[i] = 1 and recip[i] = 1 / s[i] exactly when s[i] mod L != 0; otherwise recip[i] is 32 zero bytes and
 *     ok[i] = 0 (_scalar_invert).  The one difference from libsodium: zero is judged AFTER reduction, so s = L (or any multiple of L)
 *     gives ok = 0; libsodium compares the raw bytes with zero and returns 0 for s = L.
 *   ed25519_ScalarIsCanonical_*: ok[i] = 1 exactly when s[i] < L (dalek's Scalar::from_canonical_bytes).
 *   Inputs are never written.  An output buffer may be exactly an input buffer (in place: same pointer, same n); any other overlap
 *   between an output and another argument is undefined.  Every row of every output is written.
 *   n == 0 returns 0, with or without a device; a null pointer is an argument error.  Without a device every other call fails with
 *   an error code and c25519_amd_last_error()'s text: there is no CPU result.  *_dev forms never synchronise and take 16-byte
 *   aligned device pointers; *_batch forms stage through the calling thread's pipeline like their neighbours.
 *   c25519_amd_last_shape is not written.
 *   Secrecy.  Every scalar is secret.  No branch condition and no load or store address derives from a scalar's value in any of these
 *     calls: reductions, the zero test of Invert and its forced-zero output are masks; the only decisions are on the element index.
 * One lane per element at every n, one kernel per call, no scratch leased.  The element-wise calls move 96-160 bytes per element
 * behind a few hundred instructions.  ed25519_ScalarInvert_* is Bernstein-Yang division steps mod L (csrc/sc_invert.cuh: the 20
 * batches of 30 steps of the field inversion, with the cofactor update and the normalisation written for L), ~16 000 instructions
 * where a Fermat chain over the scalar product would be ~85 000, shared between the K elements of a lane by Montgomery's trick:
 * three scalar products per element plus one inversion per lane.  Tunable SC_INVERT_K: 1, 2, 4, 8 or 16; anything else is the
 * built-in choice, the smallest K that fits the lanes into one wave per SIMD (65 536 lanes), at most 8.
 * Measured (tools/scalar_rate.py, profiles/scalar_rate.txt; interleaved rounds, 20 launches back to back per figure): up to 2^16
 * elements ScalarInvert_dev is one lane's inversion, 0.027-0.030 ms a call at K = 1 (K = 2 / 4 / 8 / 16: 0.031-0.033 / 0.041 / 0.060 /
 * 0.097 ms); 2^17 takes 0.035 ms at K = 2, 2^18 0.043 ms at K = 4, 2^19 0.066 ms at K = 8, 2^20 0.099 ms at K = 8 (10.6 G/s; K = 16:
 * 0.111, K = 4: 0.132, K = 1: 0.373 ms) -- at each size the built-in K is the fastest by more than the rounds' spread (0.000-0.003 ms).
 * At 2^20 ScalarMul_dev takes 0.020 ms (52 G/s), ScalarMulAdd_dev 0.024 ms (44 G/s), ScalarReduce_dev 0.017 ms (62 G/s). */
int ed25519_ScalarReduce_batch(unsigned char *r, const unsigned char *s /* n x 64 */, size_t n);
int ed25519_ScalarReduce_dev(void *r, const void *s, size_t n, void *stream);
int ed25519_ScalarAdd_batch(unsigned char *z, const unsigned char *x, const unsigned char *y, size_t n);
int ed25519_ScalarAdd_dev(void *z, const void *x, const void *y, size_t n, void *stream);
int ed25519_ScalarSub_batch(unsigned char *z, const unsigned char *x, const unsigned char *y, size_t n);
int ed25519_ScalarSub_dev(void *z, const void *x, const void *y, size_t n, void *stream);
int ed25519_ScalarMul_batch(unsigned char *z, const unsigned char *x, const unsigned char *y, size_t n);
int ed25519_ScalarMul_dev(void *z, const void *x, const void *y, size_t n, void *stream);
int ed25519_ScalarNegate_batch(unsigned char *r, const unsigned char *s, size_t n);
int ed25519_ScalarNegate_dev(void *r, const void *s, size_t n, void *stream);
int ed25519_ScalarComplement_batch(unsigned char *r, const unsigned char *s, size_t n);
int ed25519_ScalarComplement_dev(void *r, const void *s, size_t n, void *stream);
int ed25519_ScalarMulAdd_batch(unsigned char *r, const unsigned char *a, const unsigned char *b, const unsigned char *c, size_t n);
int ed25519_ScalarMulAdd_dev(void *r, const void *a, const void *b, const void *c, size_t n, void *stream);
int ed25519_ScalarInvert_batch(unsigned char *recip, int *ok, const unsigned char *s, size_t n);
int ed25519_ScalarInvert_dev(void *recip, void *ok, const void *s, size_t n, void *stream);
int ed25519_ScalarIsCanonical_batch(int *ok, const unsigned char *s, size_t n);
int ed25519_ScalarIsCanonical_dev(void *ok, const void *s, size_t n, void *stream);

/* Hashing to the groups: messages to edwards25519 points, ristretto255 elements and scalars on the device (RFC 9380; RFC 9497) --
 * libsodium >= 1.0.19's crypto_core_ed25519_from_string[_ro] and crypto_core_ristretto255_from_string[_ro], RFC 9497's HashToGroup
 * and HashToScalar -- so that the front of an OPRF / PSI / VRF pipeline (identifiers, passwords, set elements in; group elements
 * out) is no host loop of SHA-512 calls in front of ristretto255_FromHash_*.  INTEGRATION.md maps the names.
 * All messages of a call are msg_size bytes: msg is n rows of msg_size bytes, as in ed25519_SignMessage_*; msg_size == 0 is allowed
 * and msg may then be NULL.  dst, the domain separation tag, is dst_len bytes in HOST memory in both forms, 1 <= dst_len <= 255.
 * Outputs are n x 32 bytes (ExpandMessageXmd: n x len_in_bytes).
 *   c25519_ExpandMessageXmd_*: out[i] = expand_message_xmd(msg[i], dst, len_in_bytes) of RFC 9380 section 5.3.1 with H = SHA-512
 *     (b_in_bytes = 64, s_in_bytes = 128), 1 <= len_in_bytes <= 16320 (ell <= 255).  dst_len of 0 or above 255 is an argument
 *     error: the RFC's oversize-DST hashing is not implemented.  len_in_bytes out of range is an argument error.
 *   ed25519_MapToCurve_*: p[i] = map_to_curve_elligator2_edwards25519(u) of RFC 9380 section 6.8.2 as the 32-byte Ed25519 encoding,
 *     NO cofactor cleared.  u is the 32 bytes of u[i] read little-endian with bit 255 masked, taken mod p (the rule
 *     ristretto255_FromHash_* has for its halves).  The one exceptional input is u = 0 mod p, for which the Montgomery point has
 *     y = 0: it gives the identity, 01 00 ... 00.  No u gives x = -1: (J - 1) / 2 is not a square mod p.
 *   ed25519_HashToCurve_*: edwards25519_XMD:SHA-512_ELL2_RO_ under the caller's DST.  hash_to_field(msg, 2) is 96 expander bytes,
 *     each 48-byte half big-endian mod p; two maps, one addition, times 8, encode.  The result is in the prime-order subgroup.
 *   ed25519_EncodeToCurve_*: edwards25519_XMD:SHA-512_ELL2_NU_: the same with one field element (48 bytes) and one map.
 *   ristretto255_HashToGroup_*: hash_to_ristretto255 of RFC 9380 appendix B: 64 expander bytes into ristretto255_FromHash's map.
 *     With dst = "HashToGroup-" || contextString it is RFC 9497's HashToGroup for ristretto255-SHA512.
 *   ed25519_HashToScalar_*: RFC 9497 section 4.1's rule for ristretto255: the 64 expander bytes read little-endian as a 512-bit
 *     integer, mod L; the output is canonical.  With dst = "HashToScalar-" || contextString it is RFC 9497's HashToScalar.
 *   Inputs are never written.  Every row of every output is written; a refused call writes nothing.
 *   n == 0 returns 0, with or without a device; a null pointer (msg too, unless msg_size == 0) is an argument error, "null pointer"
 *   in c25519_amd_last_error().  Without a device every other call fails with an error code and text: there is no CPU result.
 *   *_dev forms never synchronise and take 16-byte aligned device pointers (rows are msg_size and len_in_bytes apart, whatever
 *   alignment that gives them); *_batch forms stage through the calling thread's pipeline like their neighbours.
 *   c25519_amd_last_shape is not written.
 *   Secrecy.  Messages are secret (OPRF inputs, passwords), and so are the expander's output and u.  No branch condition and no load
 *     or store address derives from them: the block loops run on the lengths, every CMOV of the map, its sgn0 fix-up and its
 *     exceptional case are masks.  Lengths and the DST are public.
 * One lane per element at every n, ONE kernel per call, no scratch leased and no device memory allocated: everything that is the
 * same for the whole call -- the lengths, the DST, SHA-512's padding -- travels in the kernel's arguments (csrc/h2c25519.cuh), so a
 * *_dev call can be captured into a graph and does not touch the state other streams keep in flight.  b_0 starts from the constant
 * state behind Z_pad's block of zeros; a message of msg_size bytes costs ceil((msg_size + dst_len + 21) / 128) compressions for
 * b_0 and ceil((dst_len + 83) / 128) for each b_i.  The Edwards encoding's inversion is the lane's own (division steps).
 * Measured (tools/h2c_rate.py, profiles/h2c_rate.txt; interleaved rounds, messages of 32 bytes, DSTs of 32 / 64 bytes -- a one- and a
 * two-block b_i --, ristretto255_FromHash_dev of the same build on the same n beside each): at 2^20 HashToGroup_dev takes 2.60 / 2.69 ms
 * (403 / 390 M/s) against 2.42 ms for FromHash_dev alone, 1.07 x / 1.11 x: the expander's two / three compressions, 0.20 / 0.28 ms as
 * ExpandMessageXmd_dev of 64 bytes (5.3 / 3.7 G/s), are what it adds, as the operation counts said.  HashToCurve_dev 2.40 / 2.57 ms
 * (438 / 408 M/s: two square-root chains, one inversion, three / five compressions), EncodeToCurve_dev 1.44 / 1.53 ms (729 / 686 M/s),
 * MapToCurve_dev 1.19 ms (881 M/s), HashToScalar_dev 0.19 / 0.28 ms (5.4 / 3.7 G/s); ed25519_SignMessage_dev on the same messages:
 * 1.17 ms.  Up to 2^16 elements a call is one lane's latency: 0.21 ms for HashToGroup, 0.18-0.20 for HashToCurve, 0.11-0.12 for
 * EncodeToCurve, 0.10 for MapToCurve, 0.02-0.03 ms for HashToScalar and the expander. */
int c25519_ExpandMessageXmd_batch(unsigned char *out /* n x len_in_bytes */, const unsigned char *msg, size_t msg_size,
                                  const unsigned char *dst, size_t dst_len, size_t len_in_bytes, size_t n);
int c25519_ExpandMessageXmd_dev(void *out, const void *msg, size_t msg_size, const void *dst /* host */, size_t dst_len,
                                size_t len_in_bytes, size_t n, void *stream);
int ed25519_MapToCurve_batch(unsigned char *p, const unsigned char *u, size_t n);
int ed25519_MapToCurve_dev(void *p, const void *u, size_t n, void *stream);
int ed25519_HashToCurve_batch(unsigned char *p, const unsigned char *msg, size_t msg_size, const unsigned char *dst, size_t dst_len, size_t n);
int ed25519_HashToCurve_dev(void *p, const void *msg, size_t msg_size, const void *dst /* host */, size_t dst_len, size_t n, void *stream);
int ed25519_EncodeToCurve_batch(unsigned char *p, const unsigned char *msg, size_t msg_size, const unsigned char *dst, size_t dst_len, size_t n);
int ed25519_EncodeToCurve_dev(void *p, const void *msg, size_t msg_size, const void *dst /* host */, size_t dst_len, size_t n, void *stream);
int ristretto255_HashToGroup_batch(unsigned char *p, const unsigned char *msg, size_t msg_size, const unsigned char *dst, size_t dst_len, size_t n);
int ristretto255_HashToGroup_dev(void *p, const void *msg, size_t msg_size, const void *dst /* host */, size_t dst_len, size_t n, void *stream);
int ed25519_HashToScalar_batch(unsigned char *s, const unsigned char *msg, size_t msg_size, const unsigned char *dst, size_t dst_len, size_t n);
int ed25519_HashToScalar_dev(void *s, const void *msg, size_t msg_size, const void *dst /* host */, size_t dst_len, size_t n, void *stream);

/* A verifiable random function: ECVRF-EDWARDS25519-SHA512-ELL2 of RFC 9381 (suite string 0x04), many proofs over many keys in one
 * call -- what leader election and sortition, key transparency and NSEC5 prove once and verify in bulk.  One lane program per call
 * does what ed25519_EncodeToCurve, two ed25519_ScalarMult_noclamp, ed25519_ScalarMultBase_noclamp, ed25519_ScalarMulAdd and three
 * host hashes would: x, k and the hash prefix stay in registers from the seed to the proof, no intermediate point is encoded only
 * to be decoded again, and the proof's fields are checked as the RFC requires.
 * Constants of the suite: suite_string = 0x04; the hash_to_curve DST is "ECVRF_" || "edwards25519_XMD:SHA-512_ELL2_NU_" || 0x04
 * (40 bytes); cLen = 16, qLen = ptLen = 32; the cofactor is 8.  All inputs of a call share one alpha_size, as the hashing calls'
 * messages share msg_size: alpha is n rows of alpha_size bytes; alpha_size == 0 is allowed and alpha may then be NULL.
 *   ed25519_VRF_Prove_* (sections 5.1, 5.4.1.2, 5.4.2.2, 5.4.3): priv[i] is the reference's 64-byte private key, seed || public key.
 *     h = SHA-512(seed); x = h[0..31] clamped; Y_string = priv[i][32..63], read AS GIVEN as ed25519_SignMessage reads it: not
 *     recomputed, not checked.  H = encode_to_curve(Y_string || alpha) under the DST above (ed25519_EncodeToCurve's rule);
 *     Gamma = [x]H; k = SHA-512(h[32..63] || H_string) read little-endian mod L; U = [k]B, V = [k]H; c = the first 16 bytes of
 *     SHA-512(0x04 || 0x02 || Y_string || H_string || Gamma_string || U_string || V_string || 0x00); s = k + c x mod L.
 *     proof[i] = Gamma_string || c || s, 80 bytes, all three canonical encodings.
 *   ed25519_VRF_ProofToHash_* (5.2, 5.4.4): ok[i] = 1 exactly when bytes 0..31 of proof[i] decode canonically -- RFC 8032's decoding:
 *     ed25519_ClassifyKey's DECODES and CANONICAL -- and s < L; then beta[i] = SHA-512(0x04 || 0x03 || enc([8]Gamma) || 0x00).
 *     Otherwise ok[i] = 0 and beta[i] is 64 zero bytes.
 *   ed25519_VRF_Verify_* (5.3 with validate_key = TRUE, 5.4.5): ok[i] = 1 exactly when pk[i] decodes canonically, pk[i] is not of
 *     small order, the proof decodes as above, and with H as above, U = [s]B - [c]Y and V = [s]H - [c]Gamma the 16 bytes recomputed
 *     from (Y, H, Gamma, U, V) equal the proof's c.  Then beta[i] is as in ProofToHash; otherwise ok[i] = 0 and beta[i] is zeros.
 *     There is no torsion-freeness rule: the RFC has none (a key of mixed order is accepted when the equations hold).
 *   Inputs are never written.  Every row of every output is written; a refused call writes nothing.
 *   n == 0 returns 0, with or without a device; a null pointer (alpha too, unless alpha_size == 0) is an argument error, "null pointer"
 *   in c25519_amd_last_error().  Without a device every other call fails with an error code and text: there is no CPU result.
 *   *_dev forms never synchronise and take 16-byte aligned device pointers (rows are 80, 64, 32 and alpha_size bytes apart, whatever
 *   alignment that gives them); *_batch forms stage through the calling thread's pipeline like their neighbours.
 *   c25519_amd_last_shape is not written.
 *   Secrecy.  In Prove the seed, h, x, k and what s is computed from are secret; Y, alpha, H, Gamma, U, V and c are public.  No
 *     branch condition and no load or store address derives from a secret, with the one exception of the base comb's row fetch for
 *     [k]B, exactly as in signing; no secret is written to device memory (k's comb columns are parked in LDS, as a signing nonce's
 *     are).  Everything in Verify and ProofToHash is public.
 * One lane per element at every n, ONE kernel per call, no scratch leased and no device memory allocated (csrc/vrf25519.cuh,
 * csrc/engine_vrf.hip): a *_dev call can be captured into a graph as one node.  [x]H and [k]H walk one table of H; the three
 * encodings of a proof share one inversion, H_string and H's table another; Verify walks half-length digits for the 128 bits of c.
 * Prove runs at two waves per SIMD (249 registers), Verify at one (415), ProofToHash at two (143); none has scratch.
 * Measured (tools/vrf_rate.py, profiles/vrf_rate.txt; interleaved rounds, alpha of 32 bytes, beside each call on the same inputs in
 * the same process the composed sequence a caller had before -- EncodeToCurve_dev, two ScalarMult_noclamp_dev,
 * ScalarMultBase_noclamp_dev, ScalarMulAdd_dev, without its three host hashes -- and one ScalarMult_noclamp_dev): at 2^20 Prove_dev
 * takes 23.22 ms (45.2 M proofs/s; spread of the rounds 0.04 ms) against 25.14 ms (spread 0.04) for the composed sequence, 0.92 x, and
 * 11.41 ms for one ScalarMult_noclamp_dev, 2.03 x; Verify_dev 29.64 ms (35.4 M/s; spread 0.06), 1.18 x composed and 1.28 x Prove;
 * ProofToHash_dev 1.28 ms (817 M/s).  Up to 2^16 elements a call is one lane's latency: 1.66-1.69 ms for Prove (composed:
 * 1.87-1.92), 1.83-1.86 for Verify, 0.10 ms for ProofToHash. */
#define ed25519_vrf_proof_size  80
#define ed25519_vrf_output_size 64
int ed25519_VRF_Prove_batch(unsigned char *proof /* n x 80 */, const unsigned char *priv /* n x 64 */,
                            const unsigned char *alpha, size_t alpha_size, size_t n);
int ed25519_VRF_Prove_dev(void *proof, const void *priv, const void *alpha, size_t alpha_size, size_t n, void *stream);
int ed25519_VRF_Verify_batch(unsigned char *beta /* n x 64 */, int *ok, const unsigned char *pk, const unsigned char *proof,
                             const unsigned char *alpha, size_t alpha_size, size_t n);
int ed25519_VRF_Verify_dev(void *beta, void *ok, const void *pk, const void *proof, const void *alpha, size_t alpha_size, size_t n, void *stream);
int ed25519_VRF_ProofToHash_batch(unsigned char *beta /* n x 64 */, int *ok, const unsigned char *proof, size_t n);
int ed25519_VRF_ProofToHash_dev(void *beta, void *ok, const void *proof, size_t n, void *stream);

/* An oblivious pseudorandom function: RFC 9497's OPRF (mode 0x00) and VOPRF (mode 0x01) with ciphersuite ristretto255-SHA512, the
 * protocol the ristretto255, scalar and hashing calls above were built towards -- PSI and password hardening evaluate mode 0x00,
 * Privacy Pass issuance and any auditable server mode 0x01 with its DLEQ proof over a batch of evaluations.  contextString is
 * "OPRFV1-" || mode || "-ristretto255-SHA512"; lp(x) is I2OSP(len(x), 2) || x.  A 32-byte scalar (blind, skS, proof_rand) is read as
 * a 256-bit little-endian integer mod L.  Elements are ristretto255 encodings; the identity is 32 zero bytes.
 *   ristretto255_OPRF_Blind_* (3.3.1 / 3.3.2 Blind): blinded[i] = blind[i] * HashToGroup(input[i]) under the DST "HashToGroup-" ||
 *     contextString of `mode`, which is 0 or 1 (anything else is an argument error).  All inputs of a call share one input_size, at
 *     most 65535 (more is an argument error); 0 is allowed and input may then be NULL.  ok[i] = 0 where the result is the identity
 *     (the RFC's InvalidInputError; blind[i] = 0 mod L gives it), and blinded[i] is then zero bytes anyway.  The caller supplies the
 *     blinds: uniform, secret, one per input.
 *   ristretto255_OPRF_Finalize_* (3.3.1 Finalize; 3.3.2 Finalize behind ristretto255_VOPRF_VerifyProof): output[i] = SHA-512(lp(input[i])
 *     || lp(N) || "Finalize") with N = (1 / blind[i]) * evaluated[i]; the same for both modes.  ok[i] = 0 and 64 zero bytes where
 *     evaluated[i] does not decode or is the identity, or where blind[i] = 0 mod L.
 *   ristretto255_OPRF_BlindEvaluate_* (3.3.1 BlindEvaluate): evaluated[i] = skS * blinded[i] under ONE key for all rows, 32 bytes
 *     (device memory in the *_dev form).  ok[i] = 0 and zero bytes where blinded[i] does not decode, or where it or the result is the
 *     identity (skS = 0 mod L gives that for every row).
 *   ristretto255_VOPRF_BlindEvaluate_* (3.3.2 BlindEvaluate, 2.2.1 GenerateProof with ComputeCompositesFast): m requests over n rows;
 *     request j owns rows offsets[j] .. offsets[j+1] - 1, between 1 and 65535 of them (the RFC encodes a row's index in its proof as
 *     I2OSP(i, 2)).  offsets has m + 1 uint64 entries: host memory in the *_batch form, where offsets[0] == 0, offsets[m] == n and
 *     1 <= offsets[j+1] - offsets[j] <= 65535 are checked as argument errors; device memory in the *_dev form, where no entry is trusted (below).
 *     evaluated[i] and ok[i] are as in ristretto255_OPRF_BlindEvaluate.  proof[j] = c || s, 64 bytes: with pkS = skS * B,
 *     seed = SHA-512(lp(pkS) || lp("Seed-" || contextString)), d_i = HashToScalar(lp(seed) || I2OSP(i, 2) || lp(blinded_i) ||
 *     lp(evaluated_i) || "Composite") for the request's i-th row, M = sum d_i * blinded_i, Z = skS * M, r = proof_rand[j], t2 = r * B,
 *     t3 = r * M: c = HashToScalar(lp(pkS) || lp(M) || lp(Z) || lp(t2) || lp(t3) || "Challenge"), s = r - c * skS mod L.  HashToScalar
 *     is ed25519_HashToScalar under "HashToScalar-" || contextString.  proof_rand is the RFC's random scalar r, supplied by the
 *     caller: it MUST be uniform, secret and used for one proof only (two proofs under one r give skS away).  req_ok[j] = 0 and
 *     a zero proof where a row of the request has ok = 0; where the request is empty, longer than 65535 or not inside [0, n]; where
 *     proof_rand[j] = 0 mod L (s would be -c * skS: the bytes of 0 and of L are both refused); where skS = 0 mod L.  Other
 *     requests are not affected.  A row that no well-formed request owns gets ok = 0 and zero bytes.
 *   ristretto255_VOPRF_VerifyProof_* (2.2.2 VerifyProof with ComputeComposites): req_ok[j] = 1 exactly when the request is well formed,
 *     every one of its rows of blinded and evaluated decodes and is not the identity, c and s of proof[j] are below L, pkS decodes and
 *     is not the identity, and with M = sum d_i * blinded_i, Z = sum d_i * evaluated_i, t2 = s * B + c * pkS, t3 = s * M + c * Z the
 *     recomputed challenge equals c.
 *   ristretto255_VOPRF_scratch_bytes(m, n): the device scratch the larger of the two proof calls leases for m requests over n rows,
 *     4 * (8 * r4(10 n) + 2 * r4(n) + 32) bytes (r4: rounded up to a multiple of 4): an extended point or two a row, the request that owns
 *     each row, pkS and the seed.
 *   Differences from the RFC's one-request API: ok is per row and req_ok per request instead of an error for the call; the random
 *     scalars are the caller's; one key per call; one proof covers at most 65535 rows.  Left out: POPRF (mode 0x02), many server
 *     keys in one call, cutting one proof's rows across pipeline pieces, and a bucket-method multi-scalar multiplication for the
 *     composites (a proof's 65535 rows are below the measured crossover of the batch equation's).
 *   Malformed offsets in the *_dev forms: the request that owns a row is found by a bisection over offsets, which ends after at most
 *     32 steps and reads entries 0 .. m only whatever they hold; a request counts as well formed when offsets[j] < offsets[j+1],
 *     their difference is at most 65535 and offsets[j+1] <= n, and its proof is made or accepted only when the bisection gave every
 *     one of its rows to it.  Anything else is req_ok = 0 (and ok = 0 for the rows nobody owns), never an access outside the arrays.
 *   Inputs are never written.  Every row of every output is written; a refused call writes nothing.  n == 0 (and m == 0) returns 0,
 *   with or without a device; a null pointer is an argument error.  Without a device every other call fails with an error code and
 *   text: there is no CPU result.  *_dev forms never synchronise and take 16-byte aligned device pointers.  The three per-row
 *   *_batch forms stage through the calling thread's pipeline in pieces like their neighbours (skS is uploaded once per call); the
 *   two proof calls run as ONE piece: upload, the *_dev call, download.  The device copy of skS (the per-row form's and the proof
 *   calls') and the proof calls' whole staging, proof_rand included, are zeroed before the call returns.  input and blind of the
 *   Blind and Finalize *_batch forms travel through the pipeline's staging buffers like signing keys: those are zeroed when they are
 *   replaced or released (c25519_amd_thread_release), not per call.
 *   c25519_amd_last_shape is not written.
 *   Secrecy.  input, blind, skS, proof_rand and what is derived from them before it is published are secret; blinded, evaluated,
 *     pkS, d_i, M, Z, c and s are public.  No branch condition and no load or store address derives from a secret, with the one
 *     exception of the base comb's row fetch for skS * B and r * B in the VOPRF server, exactly as in signing.  skS and proof_rand
 *     are read from device memory where they are used and are never kernel arguments, and no secret is written to device memory:
 *     the server's scratch holds d_i * blinded_i, the request that owns each row, pkS and the seed.
 * The per-row calls are ONE kernel each, one lane per row, no scratch (csrc/oprf25519.cuh, csrc/engine_oprf.hip): Blind hands the sum
 * of the two Elligator maps to the walk as it stands, without ENCODE and DECODE in between; Finalize inverts mod L and hashes in the
 * lane.  The proof calls are three kernels on the caller's stream over one lease of scratch -- one lane for pkS and the seed, one
 * lane per row (the server: D_i = skS * C_i and d_i * C_i over ONE window table of C_i), one lane per request (the sum of its rows'
 * points, the walks, four encodings, the challenge) -- and allocate nothing else, so a call can be captured into a graph.  A
 * request's rows are summed by ONE lane: a call of many small requests fills the device, one proof over tens of thousands of rows
 * waits for that lane.
 * Every kernel is without scratch memory; the per-row kernels and both row stages run at two waves per SIMD (the server's row lane
 * builds C_i's two table rows a second time rather than keep them under the encoding of D_i; the verifier's rows take a lane per
 * point), the per-request stages at one.
 * Measured (tools/oprf_rate.py, profiles/oprf_rate.txt; interleaved rounds, inputs of 32 bytes, beside each call on the same inputs
 * in the same process the composed sequence of existing *_dev calls a caller had before, without its host hashes): at 2^20 rows
 * Blind_dev takes 13.73 ms (76.4 M/s; spread of the rounds 0.19 ms) against 14.95 ms for HashToGroup_dev + ScalarMult_dev, 0.92 x;
 * Finalize_dev 12.76 ms (82.2 M/s), 1.03 x ScalarInvert_dev + ScalarMult_dev (12.42 ms), which leaves the hashes to the host: SLOWER
 * than that sequence by 0.33 ms, its hash's price, where the sequence with the download and a per-item host SHA-512 loop behind it
 * took 626 ms; OPRF_BlindEvaluate_dev 12.24 ms (85.7 M/s), 0.99 x ScalarMult_dev with the key repeated 2^20 times (12.31 ms).
 * VOPRF_BlindEvaluate_dev over requests of 64 rows 26.23 ms (40.0 M rows/s), 0.97 x its composed sequence (two ScalarMult_dev and a
 * HashToScalar_dev per row, the per-request calls; WITHOUT the sums, which no existing call does: 27.12 ms), 2.14 x one ScalarMult_dev;
 * VOPRF_VerifyProof_dev 28.19 ms (37.2 M rows/s), 0.97 x composed.  By request size at 2^20 rows, server / verifier: requests of 1
 * row 53.7 / 67.2 ms, of 64 rows 27.1 / 28.4 ms, of 4096 rows 48.5 / 68.5 ms, of 65535 rows 249 / 600 ms -- ONE lane sums a
 * request's rows, so few large requests wait for that lane; issuance-sized requests are the case the calls are built for.  Up to
 * 2^16 rows a call is one lane's latency: 0.97-1.15 ms (Blind; composed 1.08-1.26), 0.91-1.04 (Finalize), 0.87-0.97
 * (OPRF_BlindEvaluate), 3.9-4.9 ms for the proof calls' three stages. */
#define ristretto255_oprf_output_size 64
#define ristretto255_voprf_proof_size 64
#define ristretto255_voprf_max_rows   65535
int ristretto255_OPRF_Blind_batch(unsigned char *blinded /* n x 32 */, int *ok, const unsigned char *input, size_t input_size,
                                  const unsigned char *blind /* n x 32 */, int mode, size_t n);
int ristretto255_OPRF_Blind_dev(void *blinded, void *ok, const void *input, size_t input_size, const void *blind, int mode, size_t n, void *stream);
int ristretto255_OPRF_Finalize_batch(unsigned char *output /* n x 64 */, int *ok, const unsigned char *input, size_t input_size,
                                     const unsigned char *blind, const unsigned char *evaluated, size_t n);
int ristretto255_OPRF_Finalize_dev(void *output, void *ok, const void *input, size_t input_size, const void *blind, const void *evaluated, size_t n,
                                   void *stream);
int ristretto255_OPRF_BlindEvaluate_batch(unsigned char *evaluated /* n x 32 */, int *ok, const unsigned char *skS /* 32 */,
                                          const unsigned char *blinded, size_t n);
int ristretto255_OPRF_BlindEvaluate_dev(void *evaluated, void *ok, const void *skS, const void *blinded, size_t n, void *stream);
int ristretto255_VOPRF_BlindEvaluate_batch(unsigned char *evaluated /* n x 32 */, unsigned char *proof /* m x 64 */, int *ok /* n */, int *req_ok /* m */,
                                           const unsigned char *skS /* 32 */, const unsigned char *proof_rand /* m x 32 */,
                                           const unsigned char *blinded /* n x 32 */, const uint64_t *offsets /* m + 1 */, size_t m, size_t n);
int ristretto255_VOPRF_BlindEvaluate_dev(void *evaluated, void *proof, void *ok, void *req_ok, const void *skS, const void *proof_rand,
                                         const void *blinded, const void *offsets, size_t m, size_t n, void *stream);
int ristretto255_VOPRF_VerifyProof_batch(int *req_ok /* m */, const unsigned char *pkS /* 32 */, const unsigned char *blinded /* n x 32 */,
                                         const unsigned char *evaluated /* n x 32 */, const unsigned char *proof /* m x 64 */,
                                         const uint64_t *offsets /* m + 1 */, size_t m, size_t n);
int ristretto255_VOPRF_VerifyProof_dev(void *req_ok, const void *pkS, const void *blinded, const void *evaluated, const void *proof,
                                       const void *offsets, size_t m, size_t n, void *stream);
size_t ristretto255_VOPRF_scratch_bytes(size_t m, size_t n);

/* ---- multiscalar multiplication: Q = sum_i [s_i] P_i on edwards25519 and on ristretto255 ------------------------------------------
 * What Pedersen and vector commitments, Bulletproofs-style verifiers, batched Schnorr / DLEQ / VRF checks and ElGamal are built on
 * (curve25519-dalek: the traits MultiscalarMul and VartimeMultiscalarMul).  A call computes n_groups INDEPENDENT sums of m terms each:
 * scalar and point are n_groups * m rows of 32 bytes, group g owns rows g * m .. g * m + m - 1; q is n_groups x 32 bytes, ok
 * n_groups ints.  n_groups = 1 is dalek's call, m = 2 a batch of Pedersen commitments.  Every group of a call has the same m.
 *   scalar   s_i is ALL 256 bits of the 32 bytes, little-endian, REDUCED MOD L -- how the ed25519_Scalar* calls read a scalar, NOT the
 *            "low 255 bits" of the _noclamp calls: the two flavours below must give the same bytes on an Edwards point with a torsion
 *            part ([s]P and [s mod L]P differ there), and the bucket method needs canonical scalars.
 *   points   ed25519_*: decoded by the rule of ed25519_ScalarMult_* (ZIP-215: any 32 bytes with a square root), encoded canonically;
 *            the neutral element is 01 00 .. 00.  ristretto255_*: RFC 9496 DECODE / ENCODE; the identity is 32 zero bytes.
 *   verdict  ok[g] = 1 exactly when all m points of group g decode, and then q[g] is the sum; otherwise ok[g] = 0 and q[g] is 32 zero
 *            bytes.  Other groups are not affected.  Every row of q and ok is written.
 *   errors   n_groups = 0 returns 0 and does nothing.  m = 0, a null pointer, m > 2^26 (the bucket method's index entries hold a 32-bit
 *            point index and a sign; c25519_multiscalar_max_m) or n_groups * m > 2^31 is an argument error (non-zero return, nothing
 *            written).
 *   _batch   stages the WHOLE call as one piece on one stream (a group is never cut across pipeline pieces, as with the VOPRF proof
 *            calls) through a buffer of the calling thread that is zeroed before the call returns, and returns when it is done.
 *   _dev     16-byte aligned device pointers and a stream; never synchronises, allocates nothing beyond one lease of
 *            c25519_MultiScalarMult_scratch_bytes(m, n_groups, vartime) bytes of the calling thread's work scratch (under the current
 *            tunables; 0 for sizes the calls refuse), and can be captured into a graph.
 * SECRECY.  In ed25519_MultiScalarMult_* and ristretto255_MultiScalarMult_* the scalars are secret and the points public: no branch
 * condition and no load or store address derives from a scalar -- not a table row, not a row fetch (tests/test_secret_taint_msm.py).
 * The *_vartime_* calls are for PUBLIC inputs only: THEIR RUNNING TIME AND THEIR MEMORY ACCESSES DEPEND ON THE SCALARS (bucket
 * addresses are the scalars' digits).  USE THEM ONLY WHERE EVERY SCALAR AND EVERY POINT IS PUBLIC (verification equations).
 * How it runs.  Constant-time path (the plain calls at every size): one lane per row reduces the scalar, decodes the point and runs
 * the group calls' variable-base walk (table in registers, rows selected by masks), leaving an extended point and a decode flag in
 * scratch -- no encoding, no inversion; then passes in which one lane adds at most 64 consecutive points of a group by the complete
 * addition (equal and opposite points need no case of their own) and ANDs their flags, until a group has one point: a group of 2^20
 * rows is three short passes; then one lane per group: the Edwards encoding behind the shared inversion, the ristretto255 one in the
 * lane.  Variable-time path (the _vartime calls with m >= MSM_BUCKET_MIN): the bucket method of ed25519_VerifyBatch_zip215_* per
 * group, one group after the other over the same scratch -- packed rows of the points P_i themselves (nothing is negated), scalars
 * reduced and biased, that call's count / scan / scatter / buckets / windows kernels unchanged, Horner over the windows and the
 * encoding.  A _vartime call below MSM_BUCKET_MIN takes the constant-time path, which is a correct implementation of its contract.
 * Tunables: MSM_BUCKET_MIN (smallest m of the bucket path for any number of groups; 0: never, 1: always; built-in: 2^10 for a call
 * of ONE group, 2^18 for more) and MSM_WINDOW (the bucket path's window width, 7..13; anything else: the built-in choice, 10 below
 * 2^14 points, 11 below 2^17, 12 from there).
 * Measured (tools/msm_rate.py, profiles/msm_rate.txt; interleaved rounds, canonical random scalars, distinct points; beside each
 * call the COMPOSED sequence a caller had before on the same inputs in the same process: ed25519_ScalarMult_noclamp_dev /
 * ristretto255_ScalarMult_dev, then log2 m rounds of *_PointAdd_dev).  2^20 rows, Edwards / ristretto255, plain call against
 * composed, ms: m = 2 11.59 / 12.01 against 12.33 / 13.48 (0.94 / 0.89 x); m = 64 11.76 / 11.85 against 13.43 / 14.99 (0.88 /
 * 0.79 x); m = 4096 13.89 / 14.03 against 14.88 / 16.47; m = 2^16 13.95 / 14.00 against 15.60 / 17.46; m = 2^18 13.74 / 13.95
 * against 15.78 / 17.80; m = 2^20 (one group) 13.82 / 13.57 against 16.00 / 17.87 (0.86 / 0.76 x): the plain call is not slower
 * than the sequence at any shape (spreads 0.02-0.43 ms), 75-91 M rows/s.  The bucket path, one group, best width against the plain
 * call (Edwards): 2^10 0.77 against 1.13 ms, 2^12 0.83 / 1.26, 2^14 0.97 / 1.30, 2^16 1.16 / 1.48, 2^17 1.44 / 2.31, 2^18 1.83 /
 * 4.13, 2^19 2.58 / 7.34, 2^20 4.18 / 13.51 ms (0.31 x; as a call of its own 4.12 ms, 255 M rows/s; ristretto255 4.21 / 13.53): it
 * wins from the smallest measured size by more than the rounds' spread (0.01-0.16 ms), and at 2^20 its 3.9 ns per point are the
 * batch equation's 3.4 (7.17 ms for 2 x 2^20 points) plus the scalars' reduction.  Widths at 2^20: c = 12 4.12 ms, 13 4.73, 11
 * 5.74, 10 14.2, 7 55.5.  Its groups run one after the other: 4 groups of 2^18 take 7.22 ms (plain 13.74), 16 groups of 2^16 19.6
 * ms (plain 13.95: slower), 256 groups of 2^12 227 ms (plain 13.89) -- hence the larger built-in threshold for more than one group;
 * shapes of more than 256 groups were not timed on that path. */
#define c25519_multiscalar_max_m 67108864   /* 2^26 */
int ed25519_MultiScalarMult_batch(unsigned char *q /* n_groups x 32 */, int *ok /* n_groups */, const unsigned char *scalar /* n_groups m x 32 */,
                                  const unsigned char *point /* n_groups m x 32 */, size_t m, size_t n_groups);
int ed25519_MultiScalarMult_dev(void *q, void *ok, const void *scalar, const void *point, size_t m, size_t n_groups, void *stream);
int ed25519_MultiScalarMult_vartime_batch(unsigned char *q, int *ok, const unsigned char *scalar, const unsigned char *point, size_t m, size_t n_groups);
int ed25519_MultiScalarMult_vartime_dev(void *q, void *ok, const void *scalar, const void *point, size_t m, size_t n_groups, void *stream);
int ristretto255_MultiScalarMult_batch(unsigned char *q, int *ok, const unsigned char *scalar, const unsigned char *point, size_t m, size_t n_groups);
int ristretto255_MultiScalarMult_dev(void *q, void *ok, const void *scalar, const void *point, size_t m, size_t n_groups, void *stream);
int ristretto255_MultiScalarMult_vartime_batch(unsigned char *q, int *ok, const unsigned char *scalar, const unsigned char *point, size_t m, size_t n_groups);
int ristretto255_MultiScalarMult_vartime_dev(void *q, void *ok, const void *scalar, const void *point, size_t m, size_t n_groups, void *stream);
size_t c25519_MultiScalarMult_scratch_bytes(size_t m, size_t n_groups, int vartime);

/* n x ed25519_VerifySignature (reference :67): full Init + Check per element, distinct keys.
 * Cost depends on the INPUT, which an untrusted sender controls: a key that does not decompress onto the curve sends its
 * element through the reference's own operation order in a kernel behind the walk.  Measured at n = 2^20
 * (profiles/r06_verify_worst_case.txt): all keys on the curve 1.00 x (9.5 ms), ONE off-curve key in the batch 1.15 x (one
 * lane's latency of the reference-order path, about 1.4 ms), one per 256 elements 1.15 x, every second key 1.53 x (the
 * worst case), every key 1.46 x.  Verdicts are the reference's in every case; a caller that must bound latency can pre-screen keys
 * (ed25519_ClassifyKey_* above: bit C25519_AMD_KEY_DECODES), or keep batches from different senders apart. */
int ed25519_VerifySignature_batch(int *verdict, const unsigned char *sig, const unsigned char *pk,
                                  const unsigned char *msg, size_t msg_size, size_t n);
int ed25519_VerifySignature_dev(void *verdict, const void *sig, const void *pk, const void *msg,
                                size_t msg_size, size_t n, void *stream);

int ed25519_VerifySignature_ragged_batch(int *verdict, const unsigned char *sig, const unsigned char *pk,
                                         const unsigned char *msgs, const uint64_t *offsets, size_t n);
int ed25519_VerifySignature_ragged_dev(void *verdict, const void *sig, const void *pk, const void *msgs,
                                       const uint64_t *offsets, size_t n, void *stream);

/* Strict verification: the verdict of libsodium 1.0.18's crypto_sign_verify_detached (default build), which rejects the
 * malleable and degenerate inputs the reference accepts.  Read S = sig[32..63], y_R = sig[0..31] and y_A = pk as little-endian
 * integers, bit 255 cleared from y_R and y_A; Y_small = {0, 1, p - 1, y8, p - y8}, y8 the y of a point of order 8.  The
 * verdict is 1 exactly when
 *   1. S < L;
 *   2. y_A < p (a canonical key);
 *   3. y_A mod p is not in Y_small (no key of small order);
 *   4. the key decodes onto the curve;
 *   5. y_R mod p is not in Y_small, over all 255-bit values (so p and p + 1 count);
 *   6. the plain call's verdict is 1 (cofactorless: enc(S*B - h*A) equals R byte for byte).
 * Mixed-order keys a*B + T are accepted when the signature is right, as in libsodium.
 *   Plain calls (ed25519_VerifySignature_*, the reference): rule 6 only -- (R, S + L) verifies wherever (R, S) does, and keys and
 *   R of small order, non-canonical keys and keys off the curve are taken as they are.
 *   OpenSSL 3.0 (EVP_DigestVerify, 3.0.2): rules 1, 4 and 6; it accepts keys and R of small order and keys with y >= p.
 * The rules are decided inside the lattice path's kernels (csrc/strict25519.cuh): an element that breaks one gets verdict 0
 * there and never goes to the reference-order kernel, so a key off the curve costs no more than an honest one
 * (c25519_amd_verify_last_slow_elements reports 0 for it).  The tunable VERIFY_REFERENCE_ORDER does not apply.  Argument
 * rules, dispatch and the other tunables are ed25519_VerifySignature_*'s. */
int ed25519_VerifySignature_strict_batch(int *verdict, const unsigned char *sig, const unsigned char *pk,
                                         const unsigned char *msg, size_t msg_size, size_t n);
int ed25519_VerifySignature_strict_dev(void *verdict, const void *sig, const void *pk, const void *msg,
                                       size_t msg_size, size_t n, void *stream);
int ed25519_VerifySignature_strict_ragged_batch(int *verdict, const unsigned char *sig, const unsigned char *pk,
                                                const unsigned char *msgs, const uint64_t *offsets, size_t n);
int ed25519_VerifySignature_strict_ragged_dev(void *verdict, const void *sig, const void *pk, const void *msgs,
                                              const uint64_t *offsets, size_t n, void *stream);

/* ZIP-215 verification: the rule a consensus verifier implements to the bit (Zcash since Canopy, ed25519-zebra,
 * ed25519-consensus) -- the cofactored equation, every point encoding that decodes, only S canonical.  Read S = sig[32..63] as a
 * 256-bit little-endian integer.  Decode a 32-byte string E as: sign = bit 255, y = the low 255 bits reduced mod p (all of
 * [p, 2^255) accepted), x = the square root of (y^2 - 1) / (d y^2 + 1) with parity sign; decoding fails only when there is no
 * square root, and x = 0 with sign = 1 decodes to x = 0.  The verdict is 1 exactly when
 *   1. S < L;
 *   2. the key bytes decode to a curve point A;
 *   3. sig[0..31] decodes to a curve point R;
 *   4. [8]([S]B - [k]A - R) is the neutral element, k = SHA-512(sig[0..31] || pk || msg) mod L over the bytes as given.
 * No small-order or canonical-encoding rule applies to A or R.  Single and batched verification cannot disagree under this rule.
 *
 *                          plain (reference)        OpenSSL 3.0              strict (libsodium)       ZIP-215
 *   S >= L                 accepted (S + L too)     rejected                 rejected                 rejected
 *   small-order A          accepted                 accepted                 rejected                 accepted
 *   small-order R          accepted if canonical    accepted if canonical    rejected                 accepted, any encoding
 *   y >= p                 key: y mod p; R: never   key: y mod p; R: never   rejected                 accepted: y mod p
 *   x = 0 with sign bit    key: x = 0; R: never     key: x = 0; R: never     rejected (small order)   accepted: x = 0
 *   key off the curve      taken as it is           rejected                 rejected                 rejected
 *   mixed-order key        when h*t + j = 0 mod 8   when h*t + j = 0 mod 8   when h*t + j = 0 mod 8   whenever the signature is right
 *   torsion-shifted R      when h*t + j = 0 mod 8   when h*t + j = 0 mod 8   when h*t + j = 0 mod 8   accepted
 * (A = a*B + t*T8, R = r*B + j*T8, S = r + h*a; "R: never": the byte comparison with enc(T) cannot succeed.)
 *
 * The lattice path does not compare encodings: it walks W = [rho]([S]B - [k]A - R) with rho odd, and multiplication by rho is a
 * bijection of the group that maps the 8-torsion onto itself, so [8]W = O is rule 4: the plain walk, three doublings, the same
 * neutral test ("ZIP-215 verification"; calls above 2^15 elements hand the plain walk kernel scalars multiplied by 8
 * instead).  S >= L, a key or an R that does not decode get verdict 0 where they are
 * decoded and go to no other kernel; an element whose lattice vector does not fit the walk (practically never) is decided by a
 * cofactored reference-order kernel, and c25519_amd_verify_last_slow_elements counts only those.  The tunable
 * VERIFY_REFERENCE_ORDER does not apply.  Argument rules, layouts, dispatch (COOP_MAX, QUAD_MIN / QUAD_MAX) and stream behaviour
 * are ed25519_VerifySignature_*'s.  Rate against the plain call of the same build on the same honest inputs
 * (profiles/verify_zip215_rate.txt): 0.998 x at 2^10, 0.967 at 2^12, 0.975 at 2^14, 1.001 at 2^16, 0.987 at 2^20 (110.3 M/s); a single
 * call 127.9 us (plain 128.2); at 2^20, every second key off the curve 0.95 x the honest time, every R of small order 0.99 x. */
int ed25519_VerifySignature_zip215_batch(int *verdict, const unsigned char *sig, const unsigned char *pk,
                                         const unsigned char *msg, size_t msg_size, size_t n);
int ed25519_VerifySignature_zip215_dev(void *verdict, const void *sig, const void *pk, const void *msg,
                                       size_t msg_size, size_t n, void *stream);
int ed25519_VerifySignature_zip215_ragged_batch(int *verdict, const unsigned char *sig, const unsigned char *pk,
                                                const unsigned char *msgs, const uint64_t *offsets, size_t n);
int ed25519_VerifySignature_zip215_ragged_dev(void *verdict, const void *sig, const void *pk, const void *msgs,
                                              const uint64_t *offsets, size_t n, void *stream);

/* ZIP-215 BATCH verification: ONE equation per call (ed25519-zebra's batch::Verifier, ed25519-consensus).  For n triples and a
 * 32-byte seed, with z_i = the first 16 bytes of SHA-512(seed || le64(i)) read little-endian (i = the element's index in the call, also
 * for a host call that is cut into pieces), k_i = SHA-512(sig_i[0..31] || pk_i || msg_i) mod L and A_i, R_i decoded as the ZIP-215 calls
 * above decode them, `result` is 1 exactly when
 *   1. every element has S_i < L, a key that decodes and an R that decodes (rules 1-3 above), and
 *   2. [8]([sum z_i S_i mod L]B - sum [z_i]R_i - sum [z_i k_i mod L]A_i) is the neutral element.
 * COMPLETENESS IS EXACT: if every element's ed25519_VerifySignature_zip215_* verdict is 1, result is 1 for every seed (the sum of
 * points that [8] maps to the neutral element is mapped there too).  SOUNDNESS IS PROBABILISTIC: if any verdict is 0, result is 0
 * except with probability at most 2^-128 over a uniform seed (after [8], a bad element's defect lies in the prime-order group, the
 * z_i are 128-bit and 2^128 < L, so at most one value of its z_i cancels whatever the others sum to).  THE SEED MUST BE FRESH AND
 * UNPREDICTABLE to whoever produced the signatures: someone who knows it before choosing them can make invalid ones cancel.  Never
 * reuse one, never derive it from the batch.  A batch equation under the plain or strict rules would not be sound; there is none.
 * n == 0: result 1.  The *_dev forms never synchronise; their seed is HOST memory, read before the call returns (it travels in kernel
 * arguments); a null seed is an argument error there.  result: one int in device memory, 16-byte aligned like every device pointer.
 * The *_batch forms run the same through the host pipeline -- a call cut into pieces runs one equation per piece and ANDs the results
 * -- and a null seed means 32 bytes from getrandom(2).  verdict (NULL or n ints): all ones when the result is 1; when it is 0 the call
 * runs ed25519_VerifySignature_zip215_batch on the same inputs and returns its verdicts (the fallback every consumer of a batch
 * verifier writes by hand).  With verdict == NULL only *all_valid is written.
 * Device path (csrc/engine_batch_eq.hip, DESIGN.md "ZIP-215 batch equation"): a bucket-method multi-scalar multiplication over the 2n
 * decoded points -- signed c-bit digits, a counting sort of (point, sign) by (window, bucket), one lane per bucket, running sums per
 * window -- plus one walk of the wide base comb.  Tunables: BATCH_EQ_MIN, the smallest n (of a call, or of a piece of a host call) that
 * runs the equation; smaller ones run ed25519_VerifySignature_zip215_dev into scratch and AND the verdicts (0 = never the equation,
 * 1 = always); BATCH_EQ_WINDOW, c = 7..13 (anything else: the built-in choice by n).
 * Measured on MI355X, honest inputs, device-resident (profiles/verify_batch_rate.txt; per-element path / best equation, ms):
 * 2^16 0.82 / 1.67, 2^17 1.45 / 1.98, 2^18 2.74 / 2.74, 2^19 5.11 / 4.16, 2^20 9.77 / 7.17 (1.36 x; 146 M signatures/s).  Hence BATCH_EQ_MIN defaults to
 * 2^19 = 524288, the smallest measured size from which the equation wins by more than the rounds' spread (2^18 is a tie), and the
 * built-in width is c = 10 below 2^16 elements and c = 13 from there (the fastest measured one; c = 8 ties at 2^10).  Below that the
 * equation is a chain of eight launches with a sequential tail of 0.94 ms, against 0.3-2.7 ms for the whole per-element pass.
 * WHAT A HOST CALL GETS with the default tunables: the pipeline cuts a *_batch call into pieces of n / 8 rows (not below 2^16), and
 * each piece decides for itself, so only a call of 2^22 elements or more runs the equation; a smaller one runs the per-element kernels
 * plus the AND -- the same result, the same verdict fallback, at ed25519_VerifySignature_zip215_batch's rate.  Ragged host calls are one
 * piece and run the equation from 2^19.  A caller with 2^19 .. 2^22 elements who wants the equation uses the *_dev form (or lowers
 * BATCH_EQ_MIN).  One call takes at most 2^26 elements (the equation's index entries are addressed with 32 bits): a larger n is an
 * argument error of every form and of the hook. */
int ed25519_VerifyBatch_zip215_dev(void *result, const void *sig, const void *pk, const void *msg, size_t msg_size, size_t n,
                                   const unsigned char *seed, void *stream);
int ed25519_VerifyBatch_zip215_ragged_dev(void *result, const void *sig, const void *pk, const void *msgs, const uint64_t *offsets,
                                          size_t n, const unsigned char *seed, void *stream);
int ed25519_VerifyBatch_zip215_batch(int *all_valid, int *verdict, const unsigned char *sig, const unsigned char *pk,
                                     const unsigned char *msg, size_t msg_size, size_t n, const unsigned char *seed);
int ed25519_VerifyBatch_zip215_ragged_batch(int *all_valid, int *verdict, const unsigned char *sig, const unsigned char *pk,
                                            const unsigned char *msgs, const uint64_t *offsets, size_t n, const unsigned char *seed);
/* did the calling thread's last ed25519_VerifyBatch_zip215_* call (the last piece of a host call) run the equation (1) or the
 * per-element path (0)?  -1: no such call. */
long c25519_amd_verify_batch_last_equation(void);
/* bytes of device scratch the equation takes for n elements at the width c it would run with (BATCH_EQ_WINDOW or the built-in choice),
 * wa = ceil(255 / c) windows for a key's scalar, wz = ceil(130 / c) for an R's, K = (wa + 1) * 2^(c-1) buckets (the R's top window has
 * buckets of its own), r4 = rounded up to 4:
 *   4 * (2n * 40 + (K + wa + 1) * 40 + n * (wa + wz) + 16 * ceil(n / 256) + r4(n) + 2 K + 4)
 * -- per element two packed 128-byte rows, two biased scalars and wa + wz index entries: 444 bytes at c = 13, 520 at c = 8; per bucket
 * 168 bytes (14.5 MB at c = 13). */
size_t ed25519_VerifyBatch_scratch_bytes(size_t n);

/* ed25519_VerifyBatch_zip215_* with COALESCED KEYS (what ed25519-zebra's and ed25519-consensus's batch verifiers do for their main
 * workload, many signatures from a small, known key set): keys is n_key x 32 raw key bytes (no context record: the equation builds no
 * tables), key_index is n x uint32, and element i's key is pk_i = keys[key_index[i]].  With z_i as above and
 * k_i = SHA-512(sig_i[0..31] || pk_i || msg_i) mod L, `result` is 1 exactly when
 *   1. every element has S_i < L, an R that decodes and a key pk_i that decodes, and
 *   2. [8]([sum z_i S_i mod L]B - sum_i [z_i]R_i - sum_j [(sum over i with key_index[i] = j of z_i k_i) mod L]A_j) is the neutral element
 * -- the terms under one key are merged, so the sum runs over K = n_key points instead of n, and every key is decoded once.
 * FOR EVERY INPUT AND SEED `result` EQUALS what ed25519_VerifyBatch_zip215_* gives on the gathered keys pk_i with that seed, and
 * completeness, soundness and the seed rule read as above.  The POINT inside [8](...) may differ from the un-coalesced one by an
 * 8-torsion point when a key has mixed order, because [a mod L]A != [a]A there; [8] removes the difference (the hook below returns the
 * coalesced point).  A key that no element names is not part of the batch: it does not affect the result, even if it does not
 * decode.  The same 32 bytes at two indices are two points.  n == 0: result 1.  A null pointer, n_key == 0 with n > 0, n > 2^26 or
 * n_key > 2^26 is an argument error.
 *   *_dev never synchronises, takes its seed from HOST memory as above and cannot check the indices: an index >= n_key rejects its
 *   element (result 0), and nothing outside keys is read.
 *   *_batch checks every index on the host: one >= n_key refuses the call before any work, all_valid and verdict untouched.  It
 *   uploads keys once per call into a device buffer of the calling thread (zeroed before it is freed by c25519_amd_thread_release() or
 *   a larger call) and runs sig, key_index and msg through the host pipeline, one equation per piece, the element index counting
 *   through the call; a null seed means getrandom(2).  verdict as above: when the result is 0 the call gathers the keys on the host
 *   and returns ed25519_VerifySignature_zip215_batch's verdicts.
 * Device path (csrc/engine_batch_eq.hip, DESIGN.md "Coalesced keys"): the points are the K keys, then the n R's; the canonical
 * a_i = z_i k_i mod L of a key's elements are added up as eight 32-bit words into eight 64-bit sums (below 2^58 with n <= 2^26;
 * integer addition: the result does not depend on the order) -- in LDS per workgroup first, then one no-return 64-bit atomic per
 * workgroup, distinct key and word --, one lane per key folds them mod L, and the digit passes, buckets, windows and tail are the
 * equation's own over N = K + n points.  Tunables: BATCH_EQ_INDEXED_MIN, with BATCH_EQ_MIN's semantics (0 = never the equation,
 * 1 = always); below it a call gathers the keys into scratch and runs ed25519_VerifySignature_zip215_dev plus the AND (an index out
 * of range still gives 0).  BATCH_EQ_WINDOW applies unchanged; the built-in width is chosen by n as above.
 * c25519_amd_verify_batch_last_equation() reports these calls too.
 * Measured on MI355X, honest inputs, device-resident, n elements over K <= 65536 keys (profiles/verify_batch_indexed_rate.txt;
 * per-element call on the gathered keys / un-indexed equation / this call, ms): 2^17 1.45-1.48 / 1.95-2.05 / 1.94-2.00,
 * 2^18 2.70-2.75 / 2.70-2.78 / 2.46-2.53, 2^19 5.12-5.17 / 4.06-4.16 / 3.38-3.51, 2^20 9.66-9.79 / 7.05-7.22 / 5.51-5.59 (1.26-1.30 x the
 * un-indexed equation, 1.73-1.78 x the per-element call; 190 M signatures/s).  Hence BATCH_EQ_INDEXED_MIN defaults to 2^18 = 262144,
 * the smallest measured size from which this call beats the per-element one by more than the rounds' spread at every measured
 * K <= 65536, and the built-in width stays the un-indexed call's (the faster one in every measured cell).  K = n -- every element
 * its own key, nothing to merge -- is the price of the accumulation: +0.25 ms over the un-indexed equation at 2^20 (7.45 against 7.21
 * ms), +0.27 at 2^19, within the spread below; such a call wins over the per-element one from 2^19 only (2^18: 2.84 against 2.71 ms).
 * What a host call gets: as above, a *_batch call is cut into pieces of n / 8 rows (not below 2^16) and each piece decides for itself,
 * so with the default tunables a host call runs the equation from 2^21 elements, a ragged host call (one piece) from 2^18. */
int ed25519_VerifyBatch_zip215_indexed_dev(void *result, const void *keys, size_t n_key, const void *key_index, const void *sig,
                                           const void *msg, size_t msg_size, size_t n, const unsigned char *seed, void *stream);
int ed25519_VerifyBatch_zip215_indexed_ragged_dev(void *result, const void *keys, size_t n_key, const void *key_index, const void *sig,
                                                  const void *msgs, const uint64_t *offsets, size_t n, const unsigned char *seed,
                                                  void *stream);
int ed25519_VerifyBatch_zip215_indexed_batch(int *all_valid, int *verdict, const unsigned char *keys, size_t n_key,
                                             const uint32_t *key_index, const unsigned char *sig, const unsigned char *msg,
                                             size_t msg_size, size_t n, const unsigned char *seed);
int ed25519_VerifyBatch_zip215_indexed_ragged_batch(int *all_valid, int *verdict, const unsigned char *keys, size_t n_key,
                                                    const uint32_t *key_index, const unsigned char *sig, const unsigned char *msgs,
                                                    const uint64_t *offsets, size_t n, const unsigned char *seed);
/* bytes of device scratch the coalesced equation takes for n elements over n_key keys (N = n_key + n points; c, wa, wz, K buckets and
 * r4 as for ed25519_VerifyBatch_scratch_bytes):
 *   4 * (N * 40 + (K + wa + 1) * 40 + n * wz + n_key * wa + 16 * ceil(n / 256) + 16 * n_key + r4(N) + 2 K + 4)
 * -- per element one packed row, one biased scalar, wz index entries and a flag: 204 bytes at c = 13; per key the same plus wa index
 * entries and eight 64-bit sums: 308 bytes at c = 13. */
size_t ed25519_VerifyBatch_indexed_scratch_bytes(size_t n, size_t n_key);

/* ed25519_VerifySignature_* decide every element whose key decompresses onto the curve with an exact
 * lattice-shortened walk (csrc/verify_fast.cuh, ~134 doublings instead of 255) and run the reference's own operation
 * order only for the others (set C25519_AMD_VERIFY_REFERENCE_ORDER=1 to force it for everything).  This reports how many
 * elements of the calling thread's last verification on the current device took the reference-order kernel; -1 when
 * there is nothing to report (a *_batch call that was cut into pieces reports one of its pieces).  Synchronises with
 * that call's stream. */
long c25519_amd_verify_last_slow_elements(void);
/* did the calling thread's last ed25519_Verify_Check_* call on this device walk the two wide combs (1) or did the reference-order
 * kernel decide it (0)?  -1: no such call.  Synchronises with that call's stream. */
long c25519_amd_verify_check_last_wide(void);
/* which kernel form did the calling thread's last base call take?  Written by curve25519_dh_CreateSharedKey_* /
 * _CalculatePublicKey_* (ladder and _fast), ed25519_CreateKeyPair_*, ed25519_SignMessage_* (blinded or not) and
 * ed25519_VerifySignature_*, where the dispatch decides from n (and, inside a *_batch call, from the whole call's n); a *_batch call
 * that was cut into pieces reports its last piece.  The low byte is the form:
 *   1  one element per workgroup (one, two or three waves);
 *   2  four lanes per element;
 *   3  one lane per element with no inversion launch of its own (X25519: ladder and shared inversion in ONE launch; verification:
 *      the lattice walk, which needs none);
 *   4  one lane per element, then the shared inversion as a launch of its own;
 * bits 8 and up are the lanes per workgroup of the form's main kernel (the ladder, the comb walk, the verification walk).
 * -1: no such call yet, or c25519_amd_thread_release() since.  Does not synchronise: the value is the host's. */
long c25519_amd_last_shape(void);

/* bytes of device scratch ed25519_VerifySignature_dev needs for n elements; the library allocates and caches it per host thread
 * (about 2.8 KB per element; r4 = rounded up to 4):
 *   4 * (n * 640 + 4 * r4(10 n) + r4(14 n) + 2 * r4(5 n) + 5 * r4(n) + 4)
 * -- per element the per-lane tables (640 words: the reference order's 4-fold table, the larger of the two paths' formats), the
 * projective result with its prefix products (4 x 10 words), the lattice path's scalars (14 + 5 + 5 words), its flag, slow-list and
 * order words and two point flags; four counter words per call. */
size_t ed25519_VerifySignature_scratch_bytes(size_t n);

/* Two-phase verification (reference include/ed25519_signature.h:77-93): one key, many signatures.
 * A context is 2080 bytes -- the reference's EDP_SIGV_CTX size: the 32-byte key followed by the 16-row
 * 4-fold table of 2^(64i)*(-A) subset sums, four canonical 32-byte field elements per row.
 *   Verify_Init_batch / _dev : n keys -> n contexts (n x 2080 bytes)
 *   Verify_Check_batch / _dev: ONE context, n (signature, message) pairs -> n verdicts; this is the
 *                              amortised path, the per-key table is staged in LDS.  From 2^16 pairs per call (tunable
 *                              ONE_KEY_WIDE) a context that is byte for byte Verify_Init's, for a key on the curve, is
 *                              verified over two wide fixed-base combs instead -- the base point's and one generated for the
 *                              key (0.6 ms; kept, with the context it belongs to, in 2 MiB of device memory per calling
 *                              thread until the thread exits or calls c25519_amd_thread_release(), so the next call with
 *                              the same context skips it): the same verdicts at 2.6 x the rate; any other context keeps
 *                              the first kernel, which reads the context's rows as they are, as the reference does. */
int ed25519_Verify_Init_batch(void *ctx, const unsigned char *pk, size_t n);
int ed25519_Verify_Init_dev(void *ctx, const void *pk, size_t n, void *stream);
int ed25519_Verify_Check_batch(int *verdict, const void *ctx, const unsigned char *sig,
                               const unsigned char *msg, size_t msg_size, size_t n);
int ed25519_Verify_Check_dev(void *verdict, const void *ctx, const void *sig, const void *msg,
                             size_t msg_size, size_t n, void *stream);
/* ed25519_Verify_Check_* under the strict rules 1-6 (above ed25519_VerifySignature_strict_batch): rules 2-4 apply to the context's
 * key bytes 0..31; rule 6 is ed25519_Verify_Check_*'s verdict, whose kernels read the rows as they are.  One kernel behind those
 * applies rules 1-5 (each of its workgroups decides the key itself): it adds 26-46 us per call (profiles/verify_strict_rate.txt). */
int ed25519_Verify_Check_strict_batch(int *verdict, const void *ctx, const unsigned char *sig,
                                      const unsigned char *msg, size_t msg_size, size_t n);
int ed25519_Verify_Check_strict_dev(void *verdict, const void *ctx, const void *sig, const void *msg,
                                    size_t msg_size, size_t n, void *stream);
/* n x ed25519_Verify_Check(ctxs + 2080 * ctx_index[i], sig_i, msg_i): MANY contexts in one call, a mixed stream of
 * (context, signature, message) triples in any order.  ctxs holds n_ctx records of 2080 bytes (Verify_Init's layout, read as
 * they are, like the reference: element i's verdict is what ed25519_Verify_Check_* gives for its context, tampered or not),
 * ctx_index is n x uint32.  The index is public data: its gather is not constant-time.
 *   n == 0 returns 0; a null pointer, or n_ctx == 0 with n > 0, is an argument error.
 *   *_batch checks every index on the host: one >= n_ctx refuses the call before any work, verdict untouched.
 *   *_dev cannot check without a synchronise: an index >= n_ctx gives verdict 0 and nothing outside ctxs is read.
 *   *_batch uploads the contexts once per call into a device buffer of the calling thread (zeroed before it is freed by
 *   c25519_amd_thread_release() or a larger call).  Up to COOP_MAX pairs (default 1024) run one per wave, larger calls one per
 *   lane over the contexts' rows in place (profiles/indexed_check_rate.txt). */
int ed25519_Verify_Check_indexed_batch(int *verdict, const void *ctxs, size_t n_ctx, const uint32_t *ctx_index,
                                       const unsigned char *sig, const unsigned char *msg, size_t msg_size, size_t n);
int ed25519_Verify_Check_indexed_dev(void *verdict, const void *ctxs, size_t n_ctx, const void *ctx_index,
                                     const void *sig, const void *msg, size_t msg_size, size_t n, void *stream);
int ed25519_Verify_Check_indexed_ragged_batch(int *verdict, const void *ctxs, size_t n_ctx, const uint32_t *ctx_index,
                                              const unsigned char *sig, const unsigned char *msgs, const uint64_t *offsets, size_t n);
int ed25519_Verify_Check_indexed_ragged_dev(void *verdict, const void *ctxs, size_t n_ctx, const void *ctx_index,
                                            const void *sig, const void *msgs, const uint64_t *offsets, size_t n, void *stream);

/* The ZIP-215 verdict (rules 1-4 above ed25519_VerifySignature_zip215_batch) against Verify_Init contexts: one context, or many
 * contexts and a mixed stream of triples.  Argument lists, layouts, argument errors, the host-side index check, the once-per-call
 * context upload, stream behaviour and n == 0 are those of the plain calls they are named after; contexts are ed25519_Verify_Init_*'s
 * 2080-byte records (no new context type, no new Init call).
 *   Contract: for a context that is byte for byte what Verify_Init writes for its first 32 bytes, element i's verdict equals
 *   ed25519_VerifySignature_zip215_*'s for (sig_i, those 32 bytes, msg_i) -- for every input: small-order, mixed-order,
 *   non-canonical and undecodable keys and R's included.  Any other context is the caller's own trusted storage, as for the plain
 *   calls: its verdict is unspecified (0 or 1), and nothing outside ctxs is read.  *_dev: an index >= n_ctx gives verdict 0;
 *   *_batch: such an index refuses the call before any work, verdict untouched.
 * How: the plain calls' own walk kernels leave T = [S]B - [k]A; rule 4, [8](T - R) = O, says that R lies in the coset T + E[8], so
 * R's bytes are compared with the eight points T + t -- y_R = (low 255 bits) mod p against their y, bit 255 against the parity of
 * their x (ignored for x = 0) -- behind ONE shared inversion per element: no square root of R, no extra doublings
 * (csrc/verify_ctx_zip215.cuh).  Rule 2 is decided once per context from its row 1 (the curve equation), rule 1 per pair.
 * Dispatch: calls of at least ZIP215_CHECK_MIN pairs (tunable; default 2^16; 0 = always) walk the contexts one pair per lane --
 * one context: the shared-table kernel, or the two wide combs from ONE_KEY_WIDE pairs or with a remembered comb (kept with, and
 * shared with, ed25519_Verify_Check_*'s; c25519_amd_verify_check_last_wide() reports it; the four-lane kernel of the plain call's
 * 2^10..2^14 range is not used).  Smaller calls gather bytes 0..31 of each element's context and run
 * ed25519_VerifySignature_zip215_dev's kernels: the same verdict by the contract.
 * Measured on MI355X (tools/verify_check_zip215_rate.py, profiles/verify_check_zip215_rate.txt): NOT MEASURED YET -- no device
 * was reached while these calls were built, so the tool has not produced its table and the default of ZIP215_CHECK_MIN is the plain
 * pair's measured crossover (csrc/engine_verify_ctx.hip: ZIP215_CHECK_MIN_DEFAULT), not this call's own.  By operation count (5 + 21
 * products and 9 canonicalisations per pair behind a walk of ~1 200 products) the context path should run within a few percent of the
 * plain context calls -- 204-219 M/s over many contexts, 646-664 M/s over one key at 2^20, about 1.8 x
 * ed25519_VerifySignature_zip215_* over many keys; that is a count, not a result. */
int ed25519_Verify_Check_zip215_batch(int *verdict, const void *ctx, const unsigned char *sig,
                                      const unsigned char *msg, size_t msg_size, size_t n);
int ed25519_Verify_Check_zip215_dev(void *verdict, const void *ctx, const void *sig, const void *msg,
                                    size_t msg_size, size_t n, void *stream);
int ed25519_Verify_Check_zip215_indexed_batch(int *verdict, const void *ctxs, size_t n_ctx, const uint32_t *ctx_index,
                                              const unsigned char *sig, const unsigned char *msg, size_t msg_size, size_t n);
int ed25519_Verify_Check_zip215_indexed_dev(void *verdict, const void *ctxs, size_t n_ctx, const void *ctx_index,
                                            const void *sig, const void *msg, size_t msg_size, size_t n, void *stream);
int ed25519_Verify_Check_zip215_indexed_ragged_batch(int *verdict, const void *ctxs, size_t n_ctx, const uint32_t *ctx_index,
                                                     const unsigned char *sig, const unsigned char *msgs, const uint64_t *offsets,
                                                     size_t n);
int ed25519_Verify_Check_zip215_indexed_ragged_dev(void *verdict, const void *ctxs, size_t n_ctx, const void *ctx_index,
                                                   const void *sig, const void *msgs, const uint64_t *offsets, size_t n, void *stream);

/* Multi-GPU (BASELINE.json north_star: "batches shard embarrassingly across the 8 GPUs of one node
 * with a single RCCL gather over xGMI") ------------------------------------------------------------------------------
 * A handle owns ONE WORKER THREAD PER DEVICE.  A call cuts the batch into contiguous shards (device d owns elements
 * [n*d/n_dev, n*(d+1)/n_dev)); every worker runs its shard through the same pinned, pieced pipeline as the single-GPU
 * *_batch functions (all devices upload over their own PCIe links at the same time, nothing is copied from or to
 * pageable memory), results stay resident on the device and are gathered to devices[0] with a grouped ncclGather (RCCL,
 * /opt/rocm/include/rccl/rccl.h:745; loaded with dlopen on first use) while a second thread on the root streams the
 * gathered rows to the caller -- piece by piece: every device cuts its shard at the same rows, a piece is gathered as soon
 * as every device has computed it and handed over while the devices compute the next ones, so only the last piece's
 * gather and download are exposed.  A handle of one device skips the gather.  With host destinations every result row of the gather mode crosses the ROOT's
 * PCIe link; c25519_amd_multi_set_gather(m, 0) leaves the gather out and lets every device hand its own rows to the
 * caller over its own link (same results; the gather is what BASELINE.json's north_star names, and the default).
 * Host pointers, synchronous, same byte layouts and results as the *_batch functions.  The handle also owns one stream and
 * one RCCL communicator per device and grow-only result buffers (zeroed before they are freed); it is not thread-safe
 * (one call at a time per handle). */
typedef struct c25519_amd_multi c25519_amd_multi;
int  c25519_amd_multi_create(c25519_amd_multi **m, const int *devices, int n_dev);   /* 1 <= n_dev <= 64 */
void c25519_amd_multi_destroy(c25519_amd_multi *m);
int  c25519_amd_multi_device_count(const c25519_amd_multi *m);
int  c25519_amd_multi_helper_threads(const c25519_amd_multi *m);  /* host threads that copy memory while a call runs */
int  c25519_amd_multi_set_gather(c25519_amd_multi *m, int on);   /* 1 (default): gather to devices[0]; 0: per-device downloads */
int curve25519_dh_CreateSharedKey_multi(c25519_amd_multi *m, unsigned char *shared, const unsigned char *pk,
                                        unsigned char *sk, size_t n);
int ed25519_SignMessage_multi(c25519_amd_multi *m, unsigned char *sig, const unsigned char *priv,
                              const unsigned char *msg, size_t msg_size, size_t n);
int ed25519_VerifySignature_multi(c25519_amd_multi *m, int *verdict, const unsigned char *sig, const unsigned char *pk,
                                  const unsigned char *msg, size_t msg_size, size_t n);

/* introspection used by tests and bench ------------------------------------------------------ */
/* copies the device-generated 256 x 96-byte 8-fold base table (canonical Y+X, Y-X, 2dT rows --
 * the content of reference source/base_folding8.h) to `out` */
int c25519_amd_base_table(unsigned char *out /* 24576 bytes */);

/* test hook: the encoded point T = s*B + h*(-A) that ed25519_Verify_Check compares with enc(R)
 * (reference source/ed25519_verify.c:309-310) instead of the verdict; device pointers, out is n x 32 bytes */
int c25519_amd_verify_point_dev(void *out, const void *sig, const void *pk, const void *msg, size_t msg_size,
                                size_t n, void *stream);
/* test hook: enc(T) of the point inside [8](...) of ed25519_VerifyBatch_zip215_*, always by the equation's kernels, for any n >= 1;
 * elements with S >= L or a key or R that does not decode are left out of the sums.  The role of c25519_amd_verify_point_dev.
 * out: 32 bytes of device memory. */
int c25519_amd_verify_batch_point_dev(void *out, const void *sig, const void *pk, const void *msg, size_t msg_size, size_t n,
                                      const unsigned char *seed, void *stream);
/* the same for ed25519_VerifyBatch_zip215_indexed_*: enc(T) of the COALESCED point -- it may differ from the hook above's on the gathered
 * keys by an 8-torsion point when a key has mixed order.  Elements with S >= L, an R or a named key that does not decode, or an index
 * >= n_key are left out of the sums. */
int c25519_amd_verify_batch_indexed_point_dev(void *out, const void *keys, size_t n_key, const void *key_index, const void *sig,
                                              const void *msg, size_t msg_size, size_t n, const unsigned char *seed, void *stream);

/* device field arithmetic on n pairs of 32-byte little-endian values taken mod p = 2^255-19 (host pointers):
 * out[i] = canonical(op(a[i], b[i])), op 0 mul, 1 square, 2 add, 3 sub, 4 inverse, 5 a^((p-5)/8),
 * 6 canonicalise, 7 (a-b)*(a+b), 8 a^2-b, 9 2a^2+(a+b)-b, 10 a+121665b, 11 9a, 12 inverse as a^(p-2) (the reference's
 * ecp_Inverse chain), 13 inverse by constant-time division steps (what op 4 and every kernel run; 0 -> 0 either way).
 * The unit-test hook for the L0 layer (the reference's ECP_SELF_TEST checks, test/curve25519_selftest.c:640-741). */
int c25519_amd_fe_selftest(unsigned char *out, const unsigned char *a, const unsigned char *b, size_t n, int op);

/* the same field code on raw limb vectors (host pointers): no conversion from bytes on the way in, so a test can put every
 * operand at the limits of the limb bound contract (csrc/fe25519.cuh).  A record in is 84 words: eight field elements as ten
 * 32-bit limbs each (radix 2^25.5), a control word, three words of padding; a record out is 72 words: four field elements'
 * limbs, then the same four as canonical little-endian words.  The ops are listed at their definitions:
 *   fe_limb_selftest     one lane per record (csrc/lanes.cuh: fe_limb_selftest_op, ops 0..18)
 *   quad_limb_selftest   four lanes per record (csrc/quad25519.cuh: quad::limb_selftest_op, ops 0..3)
 *   wave_limb_selftest   one wave per record (csrc/coop_ops.cuh: coop::limb_selftest_op, ops 0..6) */
int c25519_amd_fe_limb_selftest(unsigned *out, const unsigned *in, size_t n, int op);
int c25519_amd_quad_limb_selftest(unsigned *out, const unsigned *in, size_t n, int op);
int c25519_amd_wave_limb_selftest(unsigned *out, const unsigned *in, size_t n, int op);

/* the shared inversion of the batch kernels (k_batch_invert, csrc/batch_invert_lane.inc: Montgomery's trick over k elements per
 * lane, one inversion per quad of lanes) on its own, as one launch on `stream` (device pointers): in holds n field elements as ten 32-bit limbs each in the
 * struct-of-arrays layout of the kernels' scratch (limb w of element e at word w*n + e), out gets n x 32 bytes, the canonical
 * little-endian 1/z of each (0 for z = 0 mod p).  k <= 0: the group size the product kernels would take for n; 1..16 round down
 * to an instantiated size (1, 2, 4, 8, 12, 14, 16) as the INV_K knob does. */
int c25519_amd_batch_invert_selftest_dev(void *out, const void *in, size_t n, int k, void *stream);

/* device scalar arithmetic mod L (reference source/curve25519_order.c, unit checks test/curve25519_selftest.c:624-714):
 * a is n x 64 bytes (512-bit little-endian), b n x 32 bytes, out n x 32 bytes.
 *   op 0 canonical(a mod L)   1 raw a mod L            2 canonical(a[0..31] mod L)   3 raw a[0..31]*b
 *   op 4 raw a[0..31]+b       5 raw a[32..35]*2^256 + a[0..31]   (eco_ReduceHiWord)  6 canonical(a[0..31]*b + a[32..63])
 * "raw" = 256 bits congruent to the exact value mod L, not necessarily below L. */
int c25519_amd_sc_selftest(unsigned char *out, const unsigned char *a, const unsigned char *b, size_t n, int op);

/* fold recodings of n 32-byte scalars (reference ecp_8Folds / ecp_4Folds, source/curve25519_utils.c:144 / :125):
 * out is n x 128 bytes: the 32 8-fold columns as the fixed-base walk indexes them, the same 32 as the reference-order
 * verification walk consumes them, and the 64 4-fold columns. */
int c25519_amd_fold_selftest(unsigned char *out, const unsigned char *k, size_t n);

#ifdef __cplusplus
}
#endif
#endif
