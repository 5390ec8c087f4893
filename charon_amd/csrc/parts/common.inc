// common.inc -- error plumbing and device helpers (asm loads, hash_and_fit, mix64)
// Part of the single translation unit charon_hip.hip (included in order); not a stand-alone source.

// ------------------------------------------------------------------------------------------------
// error plumbing
// ------------------------------------------------------------------------------------------------
static thread_local std::string g_err;
static int fail(int code, const std::string &msg) { g_err = msg; return code; }
#define HIPCHK(expr)                                                                                         \
    do {                                                                                                     \
        hipError_t _e = (expr);                                                                              \
        if (_e != hipSuccess)                                                                                \
            return fail(_e == hipErrorOutOfMemory ? CHN_E_NOMEM : CHN_E_HIP,                                 \
                        std::string(#expr) + ": " + hipGetErrorString(_e));                                  \
    } while (0)

extern "C" const char *chn_last_error(void) { return g_err.c_str(); }
// The library reads no environment variable in a product build.  CHN_* switches (A/B of cache policies, LDS padding, traces, the fetch-roof
// probe's shape, skipping the row fetches ...) exist in diagnostics builds only: tools/build_diag.sh CHN_DIAG.
#ifdef CHN_DIAG
static inline const char *diag_env(const char *name) { return std::getenv(name); }
#else
static inline const char *diag_env(const char *) { return nullptr; }
#endif
extern "C" const char *chn_version(void) { return "charon_hip 0.1 (gfx950)"; }

// ------------------------------------------------------------------------------------------------
// device helpers
// ------------------------------------------------------------------------------------------------
#define WAVE 64
#define QCAP 128  // LDS minimiser queue entries per wavefront (power of two, >= 2*WAVE)

__device__ __constant__ uint64_t c_ibf_seeds[5] = {13572355802537770549ULL, 13043817825332782213ULL,
                                                   10650232656628343401ULL, 16499269484942379435ULL,
                                                   4893150838803335377ULL};

__device__ __forceinline__ uint32_t lane_id() { return threadIdx.x & (WAVE - 1); }

// Loads whose completion the KERNEL tracks instead of the compiler (cdna_hip_programming.md 5.7): hipcc does not see a
// load inside an asm statement, so it inserts no s_waitcnt for it -- the caller must wait before touching the result.
typedef unsigned int u32x4_t __attribute__((ext_vector_type(4)));
typedef unsigned int u32x2_t __attribute__((ext_vector_type(2)));
__device__ __forceinline__ u32x4_t asm_load_b128(const void *p) {
    u32x4_t v;
    asm volatile("global_load_dwordx4 %0, %1, off" : "=v"(v) : "v"(p) : "memory");
    return v;
}
__device__ __forceinline__ u32x2_t asm_load_b64(const void *p) {
    u32x2_t v;
    asm volatile("global_load_dwordx2 %0, %1, off" : "=v"(v) : "v"(p) : "memory");
    return v;
}

// seqan3 interleaved_bloom_filter::hash_and_fit (fastrange), SURVEY App. A.3
__device__ __forceinline__ uint64_t hash_and_fit_row(uint64_t x, uint64_t seed, uint64_t S, uint32_t shift) {
    x *= seed;
    x ^= x >> shift;
    x *= 11400714819323198485ULL;
    return __umul64hi(x, S);
}

// counter-based PRNG (splitmix64 finaliser) shared by the synthetic-workload kernels
__host__ __device__ __forceinline__ uint64_t mix64(uint64_t z) {
    z += 0x9E3779B97F4A7C15ULL;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ULL;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBULL;
    return z ^ (z >> 31);
}
