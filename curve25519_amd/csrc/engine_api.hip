// curve25519_amd/csrc/engine_api.hip -- library state and knobs, the argument checks of the *_dev forms, the unit-test hooks, the host-pointer *_batch
// forms (host_pipeline.hpp) and the reference's single-call prototypes
// (one of the engine's translation units: engine_common.cuh says which is which)
#include "engine_common.cuh"

using c25519_host::row_call;
using c25519_host::In;
using c25519_host::Out;
using c25519_host::InOut;

// ------------------------------------------------------------------------------------------------
// unit-test hooks (the counterpart of the reference's ECP_SELF_TEST unit checks,
// test/curve25519_selftest.c:624-741): one lane per input record, operations defined in lanes.cuh
// ------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(64) k_fe_selftest(void* out, const void* a, const void* b, size_t n, int op)
{
    const size_t i = (size_t)blockIdx.x * 64 + threadIdx.x;
    if (i >= n) return;
    u32 aw[8], bw[8], ow[8];
    load32(aw, a, i);
    load32(bw, b, i);
    fe_selftest_op(ow, aw, bw, op);
    store32(out, i, ow);
}

// op 14 (the division steps on a quad of lanes, safegcd25519.cuh): FOUR lanes per record, all on the same values
__global__ void __launch_bounds__(64) k_fe_selftest_quad(void* out, const void* a, const void* b, size_t n, int op)
{
    const size_t i = (size_t)blockIdx.x * 16 + (threadIdx.x >> 2);
    if (i >= n) return;                                   // (whole quads leave)
    u32 aw[8], bw[8], ow[8];
    load32(aw, a, i);
    load32(bw, b, i);
    fe_selftest_op(ow, aw, bw, op);
    if ((threadIdx.x & 3) == 0) store32(out, i, ow);
}

// the raw-limb hooks (lanes.cuh: fe_limb_selftest_op; quad25519.cuh / coop_ops.cuh: limb_selftest_op): a lane, a quad or a wave per record
__global__ void __launch_bounds__(64) k_fe_limb_selftest(u32* out, const u32* in, size_t n, int op)
{
    const size_t i = (size_t)blockIdx.x * 64 + threadIdx.x;
    if (i >= n) return;
    fe_limb_selftest_op(out + i * LIMB_OUT_WORDS, in + i * LIMB_IN_WORDS, op);
}

__global__ void __launch_bounds__(64) k_quad_limb_selftest(u32* out, const u32* in, size_t n, int op)
{
    const size_t i = (size_t)blockIdx.x * 16 + (threadIdx.x >> 2);
    if (i >= n) return;                                   // (whole quads leave)
    quad::limb_selftest_op(out + i * LIMB_OUT_WORDS, in + i * LIMB_IN_WORDS, op);
}

__global__ void __launch_bounds__(64) k_wave_limb_selftest(u32* out, const u32* in, size_t n, int op)
{
    __shared__ __attribute__((aligned(16))) u32 lds[coop::LDS_WORDS];
    const size_t i = blockIdx.x;
    if (i >= n) return;
    coop::limb_selftest_op(lds, coop::make_lane(threadIdx.x), out + i * LIMB_OUT_WORDS, in + i * LIMB_IN_WORDS, op);
}

__global__ void __launch_bounds__(64) k_sc_selftest(void* out, const void* a, const void* b, size_t n, int op)
{
    const size_t i = (size_t)blockIdx.x * 64 + threadIdx.x;
    if (i >= n) return;
    u32 lo[8], hi[8], aw[16], bw[8], ow[8];
    load32(lo, a, 2 * i);
    load32(hi, a, 2 * i + 1);
    load32(bw, b, i);
#pragma unroll
    for (int j = 0; j < 8; j++) { aw[j] = lo[j]; aw[8 + j] = hi[j]; }
    sc_selftest_op(ow, aw, bw, op);
    store32(out, i, ow);
}

__global__ void __launch_bounds__(64) k_fold_selftest(uint8_t* out /* n x 128 */, const void* k, size_t n)
{
    const size_t i = (size_t)blockIdx.x * 64 + threadIdx.x;
    if (i >= n) return;
    u32 kw[8];
    load32(kw, k, i);
    fold_selftest_op(out + 128 * i, kw);
}

namespace c25519_engine {

// the completion word for the LAST kernel of a call of one element, if the caller (host_pipeline.hpp: run_batch on a zero-copy
// call) is going to spin on it; taken at most once per call
DoneWord take_done_word(size_t n)
{
    ThreadState& t = tls();
    if (n != 1 || !t.done_offered || t.done_taken) return DoneWord{ nullptr, 0 };
    t.done_taken = true;
    return DoneWord{ t.done_word, ++t.done_seq };
}

// the two 32-byte records of a one-element call for the kernel's arguments (lanes.cuh: CallWords): only where the "device"
// pointers are this library's own pinned staging, which the host can read (a zero-copy call, host_pipeline.hpp)
CallWords call_words(size_t n, const void* rec0, const void* rec1)
{
    CallWords cw{};
    if (n != 1 || !c25519_host::zero_copy_call()) return cw;
    if (rec0) memcpy(cw.w, rec0, 32);
    if (rec1) memcpy(cw.w + 8, rec1, 32);
    cw.use = 1;
    return cw;
}
// ... a record of up to 64 bytes from word 0 and a message of up to 64 bytes from word 16 (the fixed-base operations)
CallWords call_record_and_message(size_t n, const void* rec, size_t rec_bytes, const void* msg, size_t msg_bytes)
{
    CallWords cw{};
    if (n != 1 || !c25519_host::zero_copy_call() || rec_bytes > 64 || msg_bytes > 64) return cw;
    memcpy(cw.w, rec, rec_bytes);
    if (msg_bytes) memcpy(cw.w + 16, msg, msg_bytes);
    cw.use = 1;
    return cw;
}

// *_dev arguments: n in range, pointers 16-byte aligned and -- unless C25519_AMD_NO_PTR_CHECK is set -- device (or
// managed) memory of the CURRENT device: a pointer of another GPU or a host pointer is an error here, not a fault
// inside a kernel.
int check_dev_args(size_t n, std::initializer_list<const void*> ptrs)
{
    static const bool check_owner_env = getenv("C25519_AMD_NO_PTR_CHECK") == nullptr;
    const bool check_owner = check_owner_env && !c25519_host::zero_copy_call();   // (a tiny *_batch call hands over this library's own pinned staging: host_pipeline.hpp)
    if (n > ((size_t)1 << 31)) return bad_arg("batch too large (n > 2^31)");
    int dev = 0;
    if (check_owner && n) C25519_TRY(hipGetDevice(&dev));
    for (const void* p : ptrs) {
        if (!p) continue;
        if (!aligned16(p)) return bad_arg("device pointers must be 16-byte aligned");
        if (!check_owner || n == 0) continue;
        hipPointerAttribute_t attr;
        if (hipPointerGetAttributes(&attr, p) != hipSuccess) {
            (void)hipGetLastError();
            return bad_arg("*_dev entry points take device pointers (this one is unknown to the HIP runtime)");
        }
        if (attr.type == hipMemoryTypeHost && c25519_host::zero_copy_call()) continue;   // the pinned staging of a tiny *_batch call (host_pipeline.hpp)
        if (attr.type != hipMemoryTypeDevice && attr.type != hipMemoryTypeManaged)
            return bad_arg("*_dev entry points take device pointers (got host memory)");
        if (attr.type == hipMemoryTypeDevice && attr.device != dev)
            return bad_arg("device pointer belongs to another device than the current one");
    }
    return 0;
}

}  // namespace c25519_engine

extern "C" {


const char* c25519_amd_version(void) { return "curve25519_amd 0.7 (gfx950)"; }
const char* c25519_amd_last_error(void) { return c25519_host::last_error().c_str(); }

int c25519_amd_device_count(void)
{
    C25519_API_CALL_OR(0);
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) { (void)hipGetLastError(); return 0; }
    return n;
}

int c25519_amd_host_register(void* p, size_t bytes)
{
    C25519_API_CALL();
    if (!p || !bytes) return bad_arg("null pointer or empty range");
    // page locking works on whole pages: a buffer that shares a page with another allocation would get that neighbour
    // locked, and unlocked, with it (the runtime aborts on the second unregister) -- so only whole pages are accepted
    if ((reinterpret_cast<uintptr_t>(p) & 4095u) || (bytes & 4095u)) return bad_arg("host_register: the buffer must start on a 4 KiB page and cover whole pages");
    C25519_TRY(hipHostRegister(p, bytes, hipHostRegisterDefault));
    return 0;
}

int c25519_amd_host_unregister(void* p)
{
    C25519_API_CALL();
    if (!p) return bad_arg("null pointer");
    C25519_TRY(hipHostUnregister(p));
    return 0;
}

// tuning / A-B knobs (capi_common.hpp: Tunable).  name = the part behind C25519_AMD_ of the environment variable that
// initialises the knob; value < 0 restores the library's built-in choice.
int c25519_amd_tunable_set(const char* name, long value)
{
    if (!name) return bad_arg("null pointer");
    for (int i = 0; i < c25519_host::T_COUNT; i++)
        if (!strcmp(name, c25519_host::tunable_names()[i])) {
            c25519_host::tunable_table()[i].store(value < 0 ? c25519_host::T_UNSET : value, std::memory_order_relaxed);
            return 0;
        }
    return bad_arg("c25519_amd_tunable_set: no such knob");
}

long c25519_amd_tunable_get(const char* name)
{
    if (name)
        for (int i = 0; i < c25519_host::T_COUNT; i++)
            if (!strcmp(name, c25519_host::tunable_names()[i])) return c25519_host::tunable((c25519_host::Tunable)i);
    return -2;
}

int c25519_amd_usable_cpus(void) { return c25519_host::usable_cpus(); }

int c25519_amd_set_device(int device)
{
    C25519_API_CALL();
    C25519_TRY(hipSetDevice(device));
    return 0;
}
// frees the calling thread's streams, staging buffers (zeroed first) and work scratch
void c25519_amd_thread_release(void)
{
    if (!c25519_host::runtime_alive().load()) return;                   // exit() has begun: the process' memory goes with it
    C25519_API_CALL_OR((void)0);
    c25519_host::helper_pool_slot().reset();              // the pipeline's parked helper threads
    tls().release();
    c25519_host::last_shape() = -1;
}
// test / accounting hook: the kernel form the calling thread's last base call took (include/curve25519_amd.h); no synchronisation,
// the dispatch wrote it on the host
long c25519_amd_last_shape(void) { return c25519_host::last_shape(); }
// ---- unit-test hooks (host pointers) ---------------------------------------------------------------
int c25519_amd_fe_selftest(unsigned char* out, const unsigned char* a, const unsigned char* b, size_t n, int op)
{
    if (!out || !a || !b) return bad_arg("null pointer");
    if (n == 0) return 0;
    return run_batch(n, { Arr{ a, nullptr, 32 }, Arr{ b, nullptr, 32 }, Arr{ nullptr, out, 32 } },
                     [&](void** d, size_t c, size_t, hipStream_t st) -> int {
                         if (op == 14) k_fe_selftest_quad<<<grid_for(c, 16), 64, 0, st>>>(d[2], d[0], d[1], c, op);
                         else k_fe_selftest<<<grid_for(c, 64), 64, 0, st>>>(d[2], d[0], d[1], c, op);
                         C25519_TRY(hipGetLastError());
                         return 0;
                     });
}

// shape 0: one lane per record, 1: a quad, 2: a wave
static int limb_selftest(unsigned* out, const unsigned* in, size_t n, int op, int shape, int ops)
{
    if (!out || !in) return bad_arg("null pointer");
    if (op < 0 || op >= ops) return bad_arg("limb self-test: no such op");
    if (n == 0) return 0;
    return run_batch(n, { Arr{ in, nullptr, 4 * LIMB_IN_WORDS }, Arr{ nullptr, out, 4 * LIMB_OUT_WORDS } },
                     [&](void** d, size_t c, size_t, hipStream_t st) -> int {
                         u32* o = static_cast<u32*>(d[1]);
                         const u32* a = static_cast<const u32*>(d[0]);
                         if (shape == 0) k_fe_limb_selftest<<<grid_for(c, 64), 64, 0, st>>>(o, a, c, op);
                         else if (shape == 1) k_quad_limb_selftest<<<grid_for(c, 16), 64, 0, st>>>(o, a, c, op);
                         else k_wave_limb_selftest<<<(unsigned)c, 64, 0, st>>>(o, a, c, op);
                         C25519_TRY(hipGetLastError());
                         return 0;
                     });
}
int c25519_amd_fe_limb_selftest(unsigned* out, const unsigned* in, size_t n, int op) { return limb_selftest(out, in, n, op, 0, 19); }
int c25519_amd_quad_limb_selftest(unsigned* out, const unsigned* in, size_t n, int op) { return limb_selftest(out, in, n, op, 1, 4); }
int c25519_amd_wave_limb_selftest(unsigned* out, const unsigned* in, size_t n, int op) { return limb_selftest(out, in, n, op, 2, 7); }

// the shared inversion alone (k_batch_invert with FinishInverse): ONE launch over device pointers, since the slot map depends on n
int c25519_amd_batch_invert_selftest_dev(void* out, const void* in, size_t n, int k, void* stream)
{
    C25519_API_CALL();
    if (!out || !in) return bad_arg("null pointer");
    if (k > INV_MAX_K) return bad_arg("batch inversion self-test: k > 16");
    if (int rc = check_dev_args(n, { out, in })) return rc;
    if (n == 0) return 0;
    const ProjScratch scr{ nullptr, nullptr, const_cast<u32*>(static_cast<const u32*>(in)), nullptr };
    return launch_invert_k(scr, n, k <= 0 ? inversion_k(n) : k, FinishInverse{ static_cast<u32*>(out) }, (hipStream_t)stream);
}

int c25519_amd_sc_selftest(unsigned char* out, const unsigned char* a, const unsigned char* b, size_t n, int op)
{
    if (!out || !a || !b) return bad_arg("null pointer");
    if (n == 0) return 0;
    return run_batch(n, { Arr{ a, nullptr, 64 }, Arr{ b, nullptr, 32 }, Arr{ nullptr, out, 32 } },
                     [&](void** d, size_t c, size_t, hipStream_t st) -> int {
                         k_sc_selftest<<<grid_for(c, 64), 64, 0, st>>>(d[2], d[0], d[1], c, op);
                         C25519_TRY(hipGetLastError());
                         return 0;
                     });
}

int c25519_amd_fold_selftest(unsigned char* out, const unsigned char* k, size_t n)
{
    if (!out || !k) return bad_arg("null pointer");
    if (n == 0) return 0;
    return run_batch(n, { Arr{ k, nullptr, 32 }, Arr{ nullptr, out, 128 } },
                     [&](void** d, size_t c, size_t, hipStream_t st) -> int {
                         k_fold_selftest<<<grid_for(c, 64), 64, 0, st>>>((uint8_t*)d[1], d[0], c);
                         C25519_TRY(hipGetLastError());
                         return 0;
                     });
}

int c25519_amd_base_table(unsigned char* out)
{
    C25519_API_CALL();
    if (!out) return bad_arg("null pointer");
    const u32* bytes = nullptr;
    if (int rc = base_tables(nullptr, &bytes)) return rc;
    C25519_TRY(hipMemcpy(out, bytes, 256 * 96, hipMemcpyDeviceToHost));
    return 0;
}

// ---- host-pointer entry points: stage, run the *_dev form, copy back (host_pipeline.hpp: row_call states a call's arrays in the
// order of its *_dev prototype; the wrappers with work of their own before the pipeline hand run_batch their lists themselves) ----

int curve25519_dh_CreateSharedKey_batch(unsigned char* shared, const unsigned char* pk, unsigned char* sk, size_t n)
{
    return row_call(n, { Out(shared, 32), In(pk, 32), InOut(sk, 32) }, curve25519_dh_CreateSharedKey_dev);
}

// the peer key has a device buffer of its own per calling thread, uploaded once per call -- and only when its bytes differ from
// what the thread uploaded last -- not once per piece
int curve25519_dh_CreateSharedKey_one_peer_batch(unsigned char* shared, const unsigned char* pk, unsigned char* sk, size_t n)
{
    C25519_API_CALL();
    if (!shared || !pk || !sk) return bad_arg("null pointer");
    if (n == 0) return 0;
    ThreadState& t = tls();
    C25519_RC(t.ensure());
    void* dpk = nullptr;
    C25519_RC(t.peer.device_copy(&dpk, pk));
    return run_batch(n, { Arr{ sk, sk, 32 }, Arr{ nullptr, shared, 32 } },
                     [&](void** d, size_t c, size_t, hipStream_t st) -> int {
                         return curve25519_dh_CreateSharedKey_one_peer_dev(d[1], dpk, d[0], c, st);
                     });
}

int curve25519_dh_Peer_Init_batch(void* ctx, const unsigned char* pk, size_t n)
{
    return row_call(n, { Out(ctx, 1600), In(pk, 32) }, curve25519_dh_Peer_Init_dev);
}

// many contexts in one call: every index is checked here (one >= n_ctx refuses the call before any work), the contexts are
// uploaded once per call into a grow-only device buffer of the calling thread (`kept`: the peer, the verification or the signer
// contexts'), the indices travel with the elements
static int indexed_prepare(void** dctxs, c25519_host::GrowArray& kept, size_t ctx_bytes, const void* ctxs, size_t n_ctx,
                           const uint32_t* ctx_index, size_t n)
{
    if (n_ctx == 0) return bad_arg("no contexts");
    if (n_ctx > ((size_t)1 << 32)) return bad_arg("more contexts than a uint32 index reaches");
    for (size_t i = 0; i < n; i++)
        if (ctx_index[i] >= n_ctx) return bad_arg("context index out of range");
    C25519_RC(tls().ensure());
    return kept.upload(dctxs, ctxs, n_ctx * ctx_bytes);
}

int curve25519_dh_CreateSharedKey_indexed_batch(unsigned char* shared, const void* ctxs, size_t n_ctx, const uint32_t* ctx_index,
                                                unsigned char* sk, size_t n)
{
    C25519_API_CALL();
    if (!shared || !ctxs || !ctx_index || !sk) return bad_arg("null pointer");
    if (n == 0) return 0;
    void* dctxs = nullptr;
    C25519_RC(indexed_prepare(&dctxs, tls().pctxs, 1600, ctxs, n_ctx, ctx_index, n));
    return run_batch(n, { Arr{ sk, sk, 32 }, Arr{ ctx_index, nullptr, sizeof(uint32_t) }, Arr{ nullptr, shared, 32 } },
                     [&](void** d, size_t c, size_t, hipStream_t st) -> int {
                         return curve25519_dh_CreateSharedKey_indexed_dev(d[2], dctxs, n_ctx, d[1], d[0], c, st);
                     });
}

int curve25519_dh_CalculatePublicKey_batch(unsigned char* pk, unsigned char* sk, size_t n)
{
    return row_call(n, { Out(pk, 32), InOut(sk, 32) }, curve25519_dh_CalculatePublicKey_dev);
}

int curve25519_dh_CalculatePublicKey_fast_batch(unsigned char* pk, unsigned char* sk, size_t n)
{
    return row_call(n, { Out(pk, 32), InOut(sk, 32) }, curve25519_dh_CalculatePublicKey_fast_dev);
}

// the blinding context of a host-pointer call: 192 bytes uploaded once per call into the thread's scratch lane
static int upload_blinding(void** dctx, const void* blinding)
{
    ThreadState& t = tls();
    C25519_RC(t.ensure());
    // a caller signs many times with one context (the reference's C++ wrapper keeps two static ones, C++/ed25519.cpp): it
    // is uploaded when its bytes differ from what this thread uploaded last, not with a synchronous copy per call
    static_assert(sizeof t.bctx.host == 4 * BLIND_WORDS, "the kept blinding record is one context");
    return t.bctx.device_copy(dctx, blinding);
}

static int keypair_batch(unsigned char* pub, unsigned char* priv, const void* blinding, const unsigned char* sk, size_t n)
{
    C25519_API_CALL();
    if (!pub || !priv || !sk) return bad_arg("null pointer");
    if (n == 0) return 0;
    void* dctx = nullptr;
    if (blinding) C25519_RC(upload_blinding(&dctx, blinding));
    return run_batch(n, { Arr{ sk, nullptr, 32 }, Arr{ nullptr, pub, 32 }, Arr{ nullptr, priv, 64 } },
                     [&](void** d, size_t c, size_t, hipStream_t st) -> int {
                         return keypair_dev(d[1], d[2], d[0], dctx, c, st);
                     });
}

int ed25519_CreateKeyPair_batch(unsigned char* pub, unsigned char* priv, const unsigned char* sk, size_t n)
{
    return keypair_batch(pub, priv, nullptr, sk, n);
}

int ed25519_CreateKeyPair_blinded_batch(unsigned char* pub, unsigned char* priv, const void* blinding,
                                        const unsigned char* sk, size_t n)
{
    if (!blinding) return bad_arg("null blinding context");
    return keypair_batch(pub, priv, blinding, sk, n);
}

static int sign_batch(unsigned char* sig, const unsigned char* priv, const void* blinding, const unsigned char* msg,
                      size_t msg_size, size_t n)
{
    C25519_API_CALL();
    if (!sig || !priv || (!msg && msg_size)) return bad_arg("null pointer");
    if (n == 0) return 0;
    void* dctx = nullptr;
    if (blinding) C25519_RC(upload_blinding(&dctx, blinding));
    return run_batch(n, { Arr{ priv, nullptr, 64 }, Arr{ msg, nullptr, msg_size }, Arr{ nullptr, sig, 64 } },
                     [&](void** d, size_t c, size_t, hipStream_t st) -> int {
                         return sign_dev(d[2], d[0], dctx, fixed_msgs(d[1], msg_size), c, st);
                     });
}

int ed25519_SignMessage_batch(unsigned char* sig, const unsigned char* priv, const unsigned char* msg,
                              size_t msg_size, size_t n)
{
    return row_call(n, { Out(sig, 64), In(priv, 64), In(msg, msg_size) }, ed25519_SignMessage_dev, msg_size);
}

int ed25519_SignMessage_blinded_batch(unsigned char* sig, const unsigned char* priv, const void* blinding,
                                      const unsigned char* msg, size_t msg_size, size_t n)
{
    if (!blinding) return bad_arg("null blinding context");
    return sign_batch(sig, priv, blinding, msg, msg_size, n);
}

int ed25519_VerifySignature_batch(int* verdict, const unsigned char* sig, const unsigned char* pk,
                                  const unsigned char* msg, size_t msg_size, size_t n)
{
    return row_call(n, { Out(verdict, sizeof(int)), In(sig, 64), In(pk, 32), In(msg, msg_size) }, ed25519_VerifySignature_dev, msg_size);
}

int ed25519_VerifySignature_strict_batch(int* verdict, const unsigned char* sig, const unsigned char* pk,
                                         const unsigned char* msg, size_t msg_size, size_t n)
{
    return row_call(n, { Out(verdict, sizeof(int)), In(sig, 64), In(pk, 32), In(msg, msg_size) }, ed25519_VerifySignature_strict_dev, msg_size);
}

int ed25519_VerifySignature_zip215_batch(int* verdict, const unsigned char* sig, const unsigned char* pk,
                                         const unsigned char* msg, size_t msg_size, size_t n)
{
    return row_call(n, { Out(verdict, sizeof(int)), In(sig, 64), In(pk, 32), In(msg, msg_size) }, ed25519_VerifySignature_zip215_dev, msg_size);
}

// ragged messages (host_pipeline.hpp: run_ragged)
int ed25519_SignMessage_ragged_batch(unsigned char* sig, const unsigned char* priv, const unsigned char* msgs,
                                     const uint64_t* offsets, size_t n)
{
    C25519_API_CALL();
    if (!sig || !priv || !offsets) return bad_arg("null pointer");
    if (n == 0) return 0;
    return run_ragged(n, { Arr{ priv, nullptr, 64 }, Arr{ nullptr, sig, 64 } }, msgs, offsets, [&](void** d, hipStream_t st) -> int {
        return sign_dev(d[1], d[0], nullptr, ragged_msgs(d[2], d[3]), n, st);
    });
}

static int verify_ragged_batch(int* verdict, const unsigned char* sig, const unsigned char* pk, const unsigned char* msgs,
                               const uint64_t* offsets, size_t n, VerifyRules rules)
{
    C25519_API_CALL();
    if (!verdict || !sig || !pk || !offsets) return bad_arg("null pointer");
    if (n == 0) return 0;
    return run_ragged(n, { Arr{ sig, nullptr, 64 }, Arr{ pk, nullptr, 32 }, Arr{ nullptr, verdict, sizeof(int) } }, msgs, offsets,
                      [&](void** d, hipStream_t st) -> int { return verify_dev(d[2], d[0], d[1], ragged_msgs(d[3], d[4]), n, st, rules); });
}

int ed25519_VerifySignature_ragged_batch(int* verdict, const unsigned char* sig, const unsigned char* pk,
                                         const unsigned char* msgs, const uint64_t* offsets, size_t n)
{
    return verify_ragged_batch(verdict, sig, pk, msgs, offsets, n, RULES_PLAIN);
}

int ed25519_VerifySignature_strict_ragged_batch(int* verdict, const unsigned char* sig, const unsigned char* pk,
                                                const unsigned char* msgs, const uint64_t* offsets, size_t n)
{
    return verify_ragged_batch(verdict, sig, pk, msgs, offsets, n, RULES_STRICT);
}

int ed25519_VerifySignature_zip215_ragged_batch(int* verdict, const unsigned char* sig, const unsigned char* pk,
                                                const unsigned char* msgs, const uint64_t* offsets, size_t n)
{
    return verify_ragged_batch(verdict, sig, pk, msgs, offsets, n, RULES_ZIP215);
}

// ---- the reference's single-call API: a device batch of one, fatal on device failure --------------

void curve25519_dh_CalculatePublicKey(unsigned char* pk, unsigned char* sk)
{
    if (int rc = curve25519_dh_CalculatePublicKey_batch(pk, sk, 1)) c25519_host::die(__func__, rc);
}

void curve25519_dh_CalculatePublicKey_fast(unsigned char* pk, unsigned char* sk)
{
    if (int rc = curve25519_dh_CalculatePublicKey_fast_batch(pk, sk, 1)) c25519_host::die(__func__, rc);
}

void curve25519_dh_CreateSharedKey(unsigned char* shared, const unsigned char* pk, unsigned char* sk)
{
    if (int rc = curve25519_dh_CreateSharedKey_batch(shared, pk, sk, 1)) c25519_host::die(__func__, rc);
}

void ed25519_CreateKeyPair(unsigned char* pubKey, unsigned char* privKey, const void* blinding, const unsigned char* sk)
{
    if (int rc = keypair_batch(pubKey, privKey, blinding, sk, 1)) c25519_host::die(__func__, rc);
}

void ed25519_SignMessage(unsigned char* signature, const unsigned char* privKey, const void* blinding,
                         const unsigned char* msg, size_t msg_size)
{
    if (int rc = sign_batch(signature, privKey, blinding, msg, msg_size, 1)) c25519_host::die(__func__, rc);
}

int ed25519_VerifySignature(const unsigned char* signature, const unsigned char* publicKey, const unsigned char* msg,
                            size_t msg_size)
{
    int verdict = 0;
    if (int rc = ed25519_VerifySignature_batch(&verdict, signature, publicKey, msg, msg_size, 1))
        c25519_host::die(__func__, rc);
    return verdict;
}

// Blinding contexts (ed25519_sign.c:289-341): 192 bytes, the reference's EDP_BLINDING_CTX shape (bl, zr, BP), derived
// ON THE DEVICE from the caller's seed; the context lives in the caller's storage or is malloc'ed here, exactly as in
// the reference.  Signing / key generation with a context computes (k + bl)*B + BP from a randomised starting point
// (lanes.cuh), so the walk and its table lookups see a scalar that differs per context; outputs are unchanged.
void* ed25519_Blinding_Init(void* context, const unsigned char* seed, size_t size)
{
    C25519_API_CALL_OR(nullptr);
    void* ctx = context ? context : malloc(4 * BLIND_WORDS);
    if (!ctx) return nullptr;                  // allocation failure is the only error the reference reports (:306)
    // a call of one through the host-pointer pipeline like every other prototype: a small seed is read in place from the pinned
    // staging, the context written there, and the call returns on the kernel's completion word (68 -> ~47 us per context)
    const int rc = run_batch(1, { Arr{ size ? seed : nullptr, nullptr, size }, Arr{ nullptr, (unsigned char*)ctx, 4 * BLIND_WORDS } },
                             [&](void** d, size_t, size_t, hipStream_t st) -> int { return ed25519_Blinding_Init_dev(d[1], d[0], size, st); });
    if (rc) c25519_host::die(__func__, rc);
    return ctx;
}

void ed25519_Blinding_Finish(void* context)
{
    if (context) {
        memset(context, 0, 4 * BLIND_WORDS);
        free(context);
    }
}

// Two-phase verification.  The context is the reference's EDP_SIGV_CTX shape (2080 bytes: pk, then 16
// rows of four canonical field elements), filled by the device; it lives in the caller's storage or is
// malloc'ed here, exactly as in the reference (ed25519_verify.c:179-237).
int ed25519_Verify_Init_batch(void* ctx, const unsigned char* pk, size_t n)
{
    return row_call(n, { Out(ctx, 2080), In(pk, 32) }, ed25519_Verify_Init_dev);
}

static int verify_check_batch(int* verdict, const void* ctx, const unsigned char* sig, const unsigned char* msg, size_t msg_size,
                              size_t n, VerifyRules rules)
{
    C25519_API_CALL();
    if (!verdict || !ctx || !sig || (!msg && msg_size)) return bad_arg("null pointer");
    if (n == 0) return 0;
    ThreadState& t = tls();
    C25519_RC(t.ensure());
    void* dctx = nullptr;                                   // (one Verify_Init and MANY Verify_Check calls on the same context: a kept record)
    C25519_RC(t.vctx.device_copy(&dctx, ctx));
    const auto check_dev = rules == RULES_STRICT ? ed25519_Verify_Check_strict_dev
                         : rules == RULES_ZIP215 ? ed25519_Verify_Check_zip215_dev : ed25519_Verify_Check_dev;
    return run_batch(n, { Arr{ sig, nullptr, 64 }, Arr{ msg, nullptr, msg_size }, Arr{ nullptr, verdict, sizeof(int) } },
                     [&](void** d, size_t c, size_t, hipStream_t st) -> int {
                         return check_dev(d[2], dctx, d[0], d[1], msg_size, c, st);
                     });
}

int ed25519_Verify_Check_batch(int* verdict, const void* ctx, const unsigned char* sig, const unsigned char* msg,
                               size_t msg_size, size_t n)
{
    return verify_check_batch(verdict, ctx, sig, msg, msg_size, n, RULES_PLAIN);
}

int ed25519_Verify_Check_strict_batch(int* verdict, const void* ctx, const unsigned char* sig, const unsigned char* msg,
                                      size_t msg_size, size_t n)
{
    return verify_check_batch(verdict, ctx, sig, msg, msg_size, n, RULES_STRICT);
}

int ed25519_Verify_Check_zip215_batch(int* verdict, const void* ctx, const unsigned char* sig, const unsigned char* msg,
                                      size_t msg_size, size_t n)
{
    return verify_check_batch(verdict, ctx, sig, msg, msg_size, n, RULES_ZIP215);
}

// (the plain and the ZIP-215 form: the same contexts in the same kept buffer, the same index check, the same pieces)
static int verify_check_indexed_batch(int* verdict, const void* ctxs, size_t n_ctx, const uint32_t* ctx_index, const unsigned char* sig,
                                      const unsigned char* msg, size_t msg_size, size_t n, bool zip215)
{
    C25519_API_CALL();
    if (!verdict || !ctxs || !ctx_index || !sig || (!msg && msg_size)) return bad_arg("null pointer");
    if (n == 0) return 0;
    void* dctxs = nullptr;
    C25519_RC(indexed_prepare(&dctxs, tls().vctxs, 2080, ctxs, n_ctx, ctx_index, n));
    const auto check_dev = zip215 ? ed25519_Verify_Check_zip215_indexed_dev : ed25519_Verify_Check_indexed_dev;
    return run_batch(n, { Arr{ sig, nullptr, 64 }, Arr{ ctx_index, nullptr, sizeof(uint32_t) }, Arr{ msg, nullptr, msg_size },
                          Arr{ nullptr, verdict, sizeof(int) } },
                     [&](void** d, size_t c, size_t, hipStream_t st) -> int {
                         return check_dev(d[3], dctxs, n_ctx, d[1], d[0], d[2], msg_size, c, st);
                     });
}

static int verify_check_indexed_ragged_batch(int* verdict, const void* ctxs, size_t n_ctx, const uint32_t* ctx_index, const unsigned char* sig,
                                             const unsigned char* msgs, const uint64_t* offsets, size_t n, bool zip215)
{
    C25519_API_CALL();
    if (!verdict || !ctxs || !ctx_index || !sig || !offsets) return bad_arg("null pointer");
    if (n == 0) return 0;
    void* dctxs = nullptr;
    C25519_RC(indexed_prepare(&dctxs, tls().vctxs, 2080, ctxs, n_ctx, ctx_index, n));
    const auto check_dev = zip215 ? ed25519_Verify_Check_zip215_indexed_ragged_dev : ed25519_Verify_Check_indexed_ragged_dev;
    return run_ragged(n, { Arr{ sig, nullptr, 64 }, Arr{ ctx_index, nullptr, sizeof(uint32_t) }, Arr{ nullptr, verdict, sizeof(int) } },
                      msgs, offsets, [&](void** d, hipStream_t st) -> int {
                          return check_dev(d[2], dctxs, n_ctx, d[1], d[0], d[3], (const uint64_t*)d[4], n, st);
                      });
}

int ed25519_Verify_Check_indexed_batch(int* verdict, const void* ctxs, size_t n_ctx, const uint32_t* ctx_index,
                                       const unsigned char* sig, const unsigned char* msg, size_t msg_size, size_t n)
{
    return verify_check_indexed_batch(verdict, ctxs, n_ctx, ctx_index, sig, msg, msg_size, n, false);
}

int ed25519_Verify_Check_indexed_ragged_batch(int* verdict, const void* ctxs, size_t n_ctx, const uint32_t* ctx_index,
                                              const unsigned char* sig, const unsigned char* msgs, const uint64_t* offsets, size_t n)
{
    return verify_check_indexed_ragged_batch(verdict, ctxs, n_ctx, ctx_index, sig, msgs, offsets, n, false);
}

int ed25519_Verify_Check_zip215_indexed_batch(int* verdict, const void* ctxs, size_t n_ctx, const uint32_t* ctx_index,
                                              const unsigned char* sig, const unsigned char* msg, size_t msg_size, size_t n)
{
    return verify_check_indexed_batch(verdict, ctxs, n_ctx, ctx_index, sig, msg, msg_size, n, true);
}

int ed25519_Verify_Check_zip215_indexed_ragged_batch(int* verdict, const void* ctxs, size_t n_ctx, const uint32_t* ctx_index,
                                                     const unsigned char* sig, const unsigned char* msgs, const uint64_t* offsets, size_t n)
{
    return verify_check_indexed_ragged_batch(verdict, ctxs, n_ctx, ctx_index, sig, msgs, offsets, n, true);
}

int ed25519_Sign_Init_batch(void* ctx, const unsigned char* priv, size_t n)
{
    return row_call(n, { Out(ctx, 128), In(priv, 64) }, ed25519_Sign_Init_dev);
}

// key classification and conversion to X25519 keys (engine_keys.hip; csrc/ed_keys.cuh)
int ed25519_ClassifyKey_batch(uint32_t* flags, const unsigned char* pk, size_t n)
{
    return row_call(n, { Out(flags, sizeof(uint32_t)), In(pk, 32) }, ed25519_ClassifyKey_dev);
}

int ed25519_PublicKey_to_X25519_batch(unsigned char* xpk, int* ok, const unsigned char* pk, size_t n)
{
    return row_call(n, { Out(xpk, 32), Out(ok, sizeof(int)), In(pk, 32) }, ed25519_PublicKey_to_X25519_dev);
}

int ed25519_PrivateKey_to_X25519_batch(unsigned char* xsk, const unsigned char* priv, size_t n)
{
    return row_call(n, { Out(xsk, 32), In(priv, 64) }, ed25519_PrivateKey_to_X25519_dev);
}

// the group operations (engine_group.hip; csrc/ed_group.cuh)
int ed25519_ScalarMult_batch(unsigned char* q, int* ok, const unsigned char* scalar, const unsigned char* point, size_t n)
{
    return row_call(n, { Out(q, 32), Out(ok, sizeof(int)), In(scalar, 32), In(point, 32) }, ed25519_ScalarMult_dev);
}

int ed25519_ScalarMult_noclamp_batch(unsigned char* q, int* ok, const unsigned char* scalar, const unsigned char* point, size_t n)
{
    return row_call(n, { Out(q, 32), Out(ok, sizeof(int)), In(scalar, 32), In(point, 32) }, ed25519_ScalarMult_noclamp_dev);
}

int ed25519_ScalarMultBase_batch(unsigned char* q, const unsigned char* scalar, size_t n)
{
    return row_call(n, { Out(q, 32), In(scalar, 32) }, ed25519_ScalarMultBase_dev);
}

int ed25519_ScalarMultBase_noclamp_batch(unsigned char* q, const unsigned char* scalar, size_t n)
{
    return row_call(n, { Out(q, 32), In(scalar, 32) }, ed25519_ScalarMultBase_noclamp_dev);
}

int ed25519_PointAdd_batch(unsigned char* r, int* ok, const unsigned char* p, const unsigned char* q, size_t n)
{
    return row_call(n, { Out(r, 32), Out(ok, sizeof(int)), In(p, 32), In(q, 32) }, ed25519_PointAdd_dev);
}

int ed25519_PointSub_batch(unsigned char* r, int* ok, const unsigned char* p, const unsigned char* q, size_t n)
{
    return row_call(n, { Out(r, 32), Out(ok, sizeof(int)), In(p, 32), In(q, 32) }, ed25519_PointSub_dev);
}

// ristretto255 (engine_ristretto.hip; csrc/ristretto255.cuh)
int ristretto255_IsValidPoint_batch(int* ok, const unsigned char* point, size_t n)
{
    return row_call(n, { Out(ok, sizeof(int)), In(point, 32) }, ristretto255_IsValidPoint_dev);
}

int ristretto255_FromHash_batch(unsigned char* p, const unsigned char* hash, size_t n)
{
    return row_call(n, { Out(p, 32), In(hash, 64) }, ristretto255_FromHash_dev);
}

int ristretto255_ScalarMult_batch(unsigned char* q, int* ok, const unsigned char* scalar, const unsigned char* point, size_t n)
{
    return row_call(n, { Out(q, 32), Out(ok, sizeof(int)), In(scalar, 32), In(point, 32) }, ristretto255_ScalarMult_dev);
}

int ristretto255_ScalarMultBase_batch(unsigned char* q, const unsigned char* scalar, size_t n)
{
    return row_call(n, { Out(q, 32), In(scalar, 32) }, ristretto255_ScalarMultBase_dev);
}

int ristretto255_PointAdd_batch(unsigned char* r, int* ok, const unsigned char* p, const unsigned char* q, size_t n)
{
    return row_call(n, { Out(r, 32), Out(ok, sizeof(int)), In(p, 32), In(q, 32) }, ristretto255_PointAdd_dev);
}

int ristretto255_PointSub_batch(unsigned char* r, int* ok, const unsigned char* p, const unsigned char* q, size_t n)
{
    return row_call(n, { Out(r, 32), Out(ok, sizeof(int)), In(p, 32), In(q, 32) }, ristretto255_PointSub_dev);
}

// the scalar field mod L (engine_scalar.hip; csrc/sc_invert.cuh)
int ed25519_ScalarReduce_batch(unsigned char* r, const unsigned char* s, size_t n)
{
    return row_call(n, { Out(r, 32), In(s, 64) }, ed25519_ScalarReduce_dev);
}

int ed25519_ScalarNegate_batch(unsigned char* r, const unsigned char* s, size_t n)
{
    return row_call(n, { Out(r, 32), In(s, 32) }, ed25519_ScalarNegate_dev);
}

int ed25519_ScalarComplement_batch(unsigned char* r, const unsigned char* s, size_t n)
{
    return row_call(n, { Out(r, 32), In(s, 32) }, ed25519_ScalarComplement_dev);
}

int ed25519_ScalarAdd_batch(unsigned char* z, const unsigned char* x, const unsigned char* y, size_t n)
{
    return row_call(n, { Out(z, 32), In(x, 32), In(y, 32) }, ed25519_ScalarAdd_dev);
}

int ed25519_ScalarSub_batch(unsigned char* z, const unsigned char* x, const unsigned char* y, size_t n)
{
    return row_call(n, { Out(z, 32), In(x, 32), In(y, 32) }, ed25519_ScalarSub_dev);
}

int ed25519_ScalarMul_batch(unsigned char* z, const unsigned char* x, const unsigned char* y, size_t n)
{
    return row_call(n, { Out(z, 32), In(x, 32), In(y, 32) }, ed25519_ScalarMul_dev);
}

int ed25519_ScalarMulAdd_batch(unsigned char* r, const unsigned char* a, const unsigned char* b, const unsigned char* c, size_t n)
{
    return row_call(n, { Out(r, 32), In(a, 32), In(b, 32), In(c, 32) }, ed25519_ScalarMulAdd_dev);
}

int ed25519_ScalarInvert_batch(unsigned char* recip, int* ok, const unsigned char* s, size_t n)
{
    return row_call(n, { Out(recip, 32), Out(ok, sizeof(int)), In(s, 32) }, ed25519_ScalarInvert_dev);
}

int ed25519_ScalarIsCanonical_batch(int* ok, const unsigned char* s, size_t n)
{
    return row_call(n, { Out(ok, sizeof(int)), In(s, 32) }, ed25519_ScalarIsCanonical_dev);
}

// hashing to the groups (engine_h2c.hip; csrc/h2c25519.cuh): the messages are staged like a signing call's, the DST stays on the host
typedef int (*h2c_dev_fn)(void*, const void*, size_t, const void*, size_t, size_t, void*);

static int h2c_batch(unsigned char* out, const unsigned char* msg, size_t msg_size, const unsigned char* dst, size_t dst_len, size_t n,
                     h2c_dev_fn call_dev)
{
    if (int rc = h2c_check_args(out, msg, msg_size, dst, dst_len, 64)) return rc;
    return row_call(n, { Out(out, 32), In(msg, msg_size) }, call_dev, msg_size, dst, dst_len);
}

int c25519_ExpandMessageXmd_batch(unsigned char* out, const unsigned char* msg, size_t msg_size, const unsigned char* dst, size_t dst_len,
                                  size_t len_in_bytes, size_t n)
{
    if (int rc = h2c_check_args(out, msg, msg_size, dst, dst_len, len_in_bytes)) return rc;
    return row_call(n, { Out(out, len_in_bytes), In(msg, msg_size) }, c25519_ExpandMessageXmd_dev, msg_size, dst, dst_len, len_in_bytes);
}

int ed25519_MapToCurve_batch(unsigned char* p, const unsigned char* u, size_t n)
{
    return row_call(n, { Out(p, 32), In(u, 32) }, ed25519_MapToCurve_dev);
}

int ed25519_HashToCurve_batch(unsigned char* p, const unsigned char* msg, size_t msg_size, const unsigned char* dst, size_t dst_len, size_t n)
{
    return h2c_batch(p, msg, msg_size, dst, dst_len, n, ed25519_HashToCurve_dev);
}

int ed25519_EncodeToCurve_batch(unsigned char* p, const unsigned char* msg, size_t msg_size, const unsigned char* dst, size_t dst_len, size_t n)
{
    return h2c_batch(p, msg, msg_size, dst, dst_len, n, ed25519_EncodeToCurve_dev);
}

int ristretto255_HashToGroup_batch(unsigned char* p, const unsigned char* msg, size_t msg_size, const unsigned char* dst, size_t dst_len, size_t n)
{
    return h2c_batch(p, msg, msg_size, dst, dst_len, n, ristretto255_HashToGroup_dev);
}

int ed25519_HashToScalar_batch(unsigned char* s, const unsigned char* msg, size_t msg_size, const unsigned char* dst, size_t dst_len, size_t n)
{
    return h2c_batch(s, msg, msg_size, dst, dst_len, n, ed25519_HashToScalar_dev);
}

// ECVRF (engine_vrf.hip; csrc/vrf25519.cuh): alpha is staged like a signing call's messages
int ed25519_VRF_Prove_batch(unsigned char* proof, const unsigned char* priv, const unsigned char* alpha, size_t alpha_size, size_t n)
{
    return row_call(n, { Out(proof, 80), In(priv, 64), In(alpha, alpha_size) }, ed25519_VRF_Prove_dev, alpha_size);
}

int ed25519_VRF_Verify_batch(unsigned char* beta, int* ok, const unsigned char* pk, const unsigned char* proof, const unsigned char* alpha,
                             size_t alpha_size, size_t n)
{
    return row_call(n, { Out(beta, 64), Out(ok, sizeof(int)), In(pk, 32), In(proof, 80), In(alpha, alpha_size) }, ed25519_VRF_Verify_dev,
                    alpha_size);
}

int ed25519_VRF_ProofToHash_batch(unsigned char* beta, int* ok, const unsigned char* proof, size_t n)
{
    return row_call(n, { Out(beta, 64), Out(ok, sizeof(int)), In(proof, 80) }, ed25519_VRF_ProofToHash_dev);
}

// OPRF and VOPRF (engine_oprf.hip; csrc/oprf25519.cuh): the inputs are staged like a signing call's messages
int ristretto255_OPRF_Blind_batch(unsigned char* blinded, int* ok, const unsigned char* input, size_t input_size, const unsigned char* blind, int mode,
                                  size_t n)
{
    if (mode != 0 && mode != 1) return bad_arg("mode must be 0 (OPRF) or 1 (VOPRF)");
    if (input_size > 65535) return bad_arg("input_size must be at most 65535");
    return row_call(n, { Out(blinded, 32), Out(ok, sizeof(int)), In(input, input_size), In(blind, 32) },
                    [=](void* b, void* o, void* in, void* bl, size_t c, hipStream_t st) -> int {
                        return ristretto255_OPRF_Blind_dev(b, o, in, input_size, bl, mode, c, st);
                    });
}

int ristretto255_OPRF_Finalize_batch(unsigned char* output, int* ok, const unsigned char* input, size_t input_size, const unsigned char* blind,
                                     const unsigned char* evaluated, size_t n)
{
    if (input_size > 65535) return bad_arg("input_size must be at most 65535");
    return row_call(n, { Out(output, 64), Out(ok, sizeof(int)), In(input, input_size), In(blind, 32), In(evaluated, 32) },
                    [=](void* out, void* o, void* in, void* bl, void* ev, size_t c, hipStream_t st) -> int {
                        return ristretto255_OPRF_Finalize_dev(out, o, in, input_size, bl, ev, c, st);
                    });
}

// the ONE key has a device buffer of its own per calling thread, uploaded once per call and zeroed when the call returns
int ristretto255_OPRF_BlindEvaluate_batch(unsigned char* evaluated, int* ok, const unsigned char* skS, const unsigned char* blinded, size_t n)
{
    C25519_API_CALL();
    if (!evaluated || !ok || !skS || !blinded) return bad_arg("null pointer");
    if (n == 0) return 0;
    ThreadState& t = tls();
    C25519_RC(t.ensure());
    void* dsk = nullptr;
    C25519_RC(t.okey.upload(&dsk, skS, 32));
    const int rc = row_call(n, { Out(evaluated, 32), Out(ok, sizeof(int)), In(blinded, 32) },
                            [=](void* ev, void* o, void* bl, size_t c, hipStream_t st) -> int {
                                return ristretto255_OPRF_BlindEvaluate_dev(ev, o, dsk, bl, c, st);
                            });
    const std::string text = c25519_host::last_error();
    const int wiped = c25519_host::zero_device_now(dsk, 32);
    if (rc) c25519_host::last_error() = text;
    return rc ? rc : wiped;
}

}  // extern "C"

// The proof calls run as ONE piece on ONE stream: every array is uploaded whole into one staging buffer of the calling thread (cut
// by the carver the scratch layouts use), `launch` gets the device pointers in list order, the outputs come back, the whole buffer
// is zeroed -- it held skS and proof_rand -- and the call returns when the stream has drained.
struct OprfStaged { const void* in; void* out; size_t bytes; };
template <size_t K, typename Launch>
static int oprf_one_piece(const OprfStaged (&arr)[K], Launch launch)
{
    ThreadState& t = tls();
    C25519_RC(t.ensure());
    hipStream_t st = t.stream[ThreadState::LANES - 1];       // the download stream, idle between pipelined calls
    Carve size;
    for (const OprfStaged& a : arr) size.take4((a.bytes + 3) / 4);
    void* base = nullptr;
    C25519_RC(t.ostage.reserve(&base, size.bytes() ? size.bytes() : 16));
    Carve cut(base);
    void* d[K];
    for (size_t i = 0; i < K; i++) d[i] = cut.take4((arr[i].bytes + 3) / 4);
    auto enqueue = [&]() -> int {
        for (size_t i = 0; i < K; i++)
            if (arr[i].in && arr[i].bytes) C25519_TRY(hipMemcpyAsync(d[i], arr[i].in, arr[i].bytes, hipMemcpyHostToDevice, st));
        C25519_RC(launch(d, st));
        for (size_t i = 0; i < K; i++)
            if (arr[i].out && arr[i].bytes) C25519_TRY(hipMemcpyAsync(arr[i].out, d[i], arr[i].bytes, hipMemcpyDeviceToHost, st));
        return 0;
    };
    const int rc = enqueue();
    const std::string text = c25519_host::last_error();
    // whatever enqueue() said: the buffer is zeroed behind what was enqueued and the stream drained (it may still be reading the
    // caller's arrays); the first failure is the call's
    const hipError_t wiped = size.bytes() ? hipMemsetAsync(base, 0, size.bytes(), st) : hipSuccess;
    const hipError_t drained = hipStreamSynchronize(st);
    if (rc) {
        (void)hipGetLastError();
        c25519_host::last_error() = text;
        return rc;
    }
    C25519_TRY(wiped);
    C25519_TRY(drained);
    return 0;
}

// offsets of a host-pointer proof call: from 0 to n in requests of 1 .. 65535 rows
static int oprf_check_offsets(const uint64_t* offsets, size_t m, size_t n)
{
    if (offsets[0] != 0 || offsets[m] != n) return bad_arg("offsets must begin at 0 and end at n");
    for (size_t j = 0; j < m; j++) {
        if (offsets[j + 1] < offsets[j]) return bad_arg("offsets must not decrease");
        if (offsets[j + 1] == offsets[j] || offsets[j + 1] - offsets[j] > 65535) return bad_arg("a request has 1 .. 65535 rows");
    }
    return 0;
}

extern "C" {

int ristretto255_VOPRF_BlindEvaluate_batch(unsigned char* evaluated, unsigned char* proof, int* ok, int* req_ok, const unsigned char* skS,
                                           const unsigned char* proof_rand, const unsigned char* blinded, const uint64_t* offsets, size_t m, size_t n)
{
    C25519_API_CALL();
    if (!skS || !offsets || (n && (!evaluated || !ok || !blinded)) || (m && (!proof || !req_ok || !proof_rand))) return bad_arg("null pointer");
    if (m > ((size_t)1 << 31) || n > ((size_t)1 << 31)) return bad_arg("batch too large (more than 2^31 requests or rows)");
    if (int rc = oprf_check_offsets(offsets, m, n)) return rc;
    if (n == 0 && m == 0) return 0;
    const OprfStaged arr[] = { { nullptr, evaluated, 32 * n }, { nullptr, proof, 64 * m }, { nullptr, ok, sizeof(int) * n }, { nullptr, req_ok, sizeof(int) * m },
                               { skS, nullptr, 32 }, { proof_rand, nullptr, 32 * m }, { blinded, nullptr, 32 * n }, { offsets, nullptr, sizeof(uint64_t) * (m + 1) } };
    return oprf_one_piece(arr, [&](void** d, hipStream_t st) -> int {
        return ristretto255_VOPRF_BlindEvaluate_dev(n ? d[0] : nullptr, m ? d[1] : nullptr, n ? d[2] : nullptr, m ? d[3] : nullptr, d[4], m ? d[5] : nullptr,
                                                    n ? d[6] : nullptr, d[7], m, n, st);
    });
}

int ristretto255_VOPRF_VerifyProof_batch(int* req_ok, const unsigned char* pkS, const unsigned char* blinded, const unsigned char* evaluated,
                                         const unsigned char* proof, const uint64_t* offsets, size_t m, size_t n)
{
    C25519_API_CALL();
    if (!pkS || !offsets || (n && (!blinded || !evaluated)) || (m && (!req_ok || !proof))) return bad_arg("null pointer");
    if (m > ((size_t)1 << 31) || n > ((size_t)1 << 31)) return bad_arg("batch too large (more than 2^31 requests or rows)");
    if (int rc = oprf_check_offsets(offsets, m, n)) return rc;
    if (m == 0) return 0;
    const OprfStaged arr[] = { { nullptr, req_ok, sizeof(int) * m }, { pkS, nullptr, 32 }, { blinded, nullptr, 32 * n }, { evaluated, nullptr, 32 * n },
                               { proof, nullptr, 64 * m }, { offsets, nullptr, sizeof(uint64_t) * (m + 1) } };
    return oprf_one_piece(arr, [&](void** d, hipStream_t st) -> int {
        return ristretto255_VOPRF_VerifyProof_dev(d[0], d[1], n ? d[2] : nullptr, n ? d[3] : nullptr, d[4], d[5], m, n, st);
    });
}

}  // extern "C"

// multiscalar multiplication (engine_msm.hip; csrc/msm_sum.cuh): ONE piece, like the proof calls -- a group is never cut across
// pipeline pieces -- through their staging buffer, which is zeroed before the call returns (the plain calls' scalars are secret)
typedef int (*msm_dev_fn)(void*, void*, const void*, const void*, size_t, size_t, void*);
static int msm_batch(unsigned char* q, int* ok, const unsigned char* scalar, const unsigned char* point, size_t m, size_t n_groups, msm_dev_fn call_dev)
{
    C25519_API_CALL();
    if (!q || !ok || !scalar || !point) return bad_arg("null pointer");
    if (m == 0) return bad_arg("m must be at least 1");
    if (m > ((size_t)1 << 26)) return bad_arg("group too large for one call (m > 2^26)");
    if (n_groups > ((size_t)1 << 31) / m) return bad_arg("batch too large (n_groups * m > 2^31)");
    if (n_groups == 0) return 0;
    const size_t rows = m * n_groups;
    const OprfStaged arr[] = { { nullptr, q, 32 * n_groups }, { nullptr, ok, sizeof(int) * n_groups }, { scalar, nullptr, 32 * rows },
                               { point, nullptr, 32 * rows } };
    return oprf_one_piece(arr, [&](void** d, hipStream_t st) -> int { return call_dev(d[0], d[1], d[2], d[3], m, n_groups, st); });
}

extern "C" {

int ed25519_MultiScalarMult_batch(unsigned char* q, int* ok, const unsigned char* scalar, const unsigned char* point, size_t m, size_t n_groups)
{
    return msm_batch(q, ok, scalar, point, m, n_groups, ed25519_MultiScalarMult_dev);
}

int ed25519_MultiScalarMult_vartime_batch(unsigned char* q, int* ok, const unsigned char* scalar, const unsigned char* point, size_t m, size_t n_groups)
{
    return msm_batch(q, ok, scalar, point, m, n_groups, ed25519_MultiScalarMult_vartime_dev);
}

int ristretto255_MultiScalarMult_batch(unsigned char* q, int* ok, const unsigned char* scalar, const unsigned char* point, size_t m, size_t n_groups)
{
    return msm_batch(q, ok, scalar, point, m, n_groups, ristretto255_MultiScalarMult_dev);
}

int ristretto255_MultiScalarMult_vartime_batch(unsigned char* q, int* ok, const unsigned char* scalar, const unsigned char* point, size_t m,
                                               size_t n_groups)
{
    return msm_batch(q, ok, scalar, point, m, n_groups, ristretto255_MultiScalarMult_vartime_dev);
}

// signatures under many signer contexts (secret: the device copy is zeroed before it is freed or replaced)
int ed25519_SignMessage_indexed_batch(unsigned char* sig, const void* ctxs, size_t n_ctx, const uint32_t* ctx_index,
                                      const unsigned char* msg, size_t msg_size, size_t n)
{
    C25519_API_CALL();
    if (!sig || !ctxs || !ctx_index || (!msg && msg_size)) return bad_arg("null pointer");
    if (n == 0) return 0;
    void* dctxs = nullptr;
    C25519_RC(indexed_prepare(&dctxs, tls().sctxs, 128, ctxs, n_ctx, ctx_index, n));
    return run_batch(n, { Arr{ ctx_index, nullptr, sizeof(uint32_t) }, Arr{ msg, nullptr, msg_size }, Arr{ nullptr, sig, 64 } },
                     [&](void** d, size_t c, size_t, hipStream_t st) -> int {
                         return ed25519_SignMessage_indexed_dev(d[2], dctxs, n_ctx, d[0], d[1], msg_size, c, st);
                     });
}

int ed25519_SignMessage_indexed_ragged_batch(unsigned char* sig, const void* ctxs, size_t n_ctx, const uint32_t* ctx_index,
                                             const unsigned char* msgs, const uint64_t* offsets, size_t n)
{
    C25519_API_CALL();
    if (!sig || !ctxs || !ctx_index || !offsets) return bad_arg("null pointer");
    if (n == 0) return 0;
    void* dctxs = nullptr;
    C25519_RC(indexed_prepare(&dctxs, tls().sctxs, 128, ctxs, n_ctx, ctx_index, n));
    return run_ragged(n, { Arr{ ctx_index, nullptr, sizeof(uint32_t) }, Arr{ nullptr, sig, 64 } }, msgs, offsets,
                      [&](void** d, hipStream_t st) -> int {
                          return ed25519_SignMessage_indexed_ragged_dev(d[1], dctxs, n_ctx, d[0], d[2], (const uint64_t*)d[3], n, st);
                      });
}

void* ed25519_Verify_Init(void* context, const unsigned char* publicKey)
{
    void* ctx = context ? context : malloc(2080);
    if (!ctx) return nullptr;                  // allocation failure is the only error the reference reports
    if (int rc = ed25519_Verify_Init_batch(ctx, publicKey, 1)) c25519_host::die(__func__, rc);
    return ctx;
}

int ed25519_Verify_Check(const void* context, const unsigned char* signature, const unsigned char* msg, size_t msg_size)
{
    int verdict = 0;
    if (int rc = ed25519_Verify_Check_batch(&verdict, context, signature, msg, msg_size, 1))
        c25519_host::die(__func__, rc);
    return verdict;
}

void ed25519_Verify_Finish(void* ctx) { free(ctx); }
}  // extern "C"
