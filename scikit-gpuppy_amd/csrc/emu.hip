// emu.hip -- fp64 products C -= A B^T emulated on the int8 matrix cores (Ozaki scheme II) for gfx950.
//
// estimate_many's deep TRSM updates (tsolve.hip, trsm_right_lt_squares) are full rectangular NT products with K = 4096 .. 32768.  fp64 MFMA
// runs at 78.6 TFLOP/s; v_mfma_i32_32x32x32_i8 retires 2048 int8 ops per clock per SIMD (~5 POPS).  Scheme II:
//   1. split   : row i of A is scaled by 2^sig_i so that |a_ik 2^sig_i| <= 2^alpha and rounded to the integer a'_ik (exact in fp64, at most
//                56 bits); likewise row j of B with tau_j and beta.  Every a'_ik is stored as its symmetric residues mod L pairwise coprime
//                moduli p_l (int8).
//   2. products: one exact int8 -> int32 GEMM per modulus (|residue| <= 128, so |sum| <= K 2^14 < 2^31 for K < 2^17), reduced mod p_l in
//                the epilogue and stored as one byte.
//   3. rebuild : per entry, the integer X = sum_k a'_ik b'_jk in [-P/2, P/2) from its L residues by the direct Chinese-remainder sum
//                X = sum_l t_l M_l - q P (t_l = r_l M_l^-1 mod p_l in fp32, the sum over 40-bit limbs of M_l = P / p_l in exact fp64
//                FMAs, q from the fp64 value of the sum, one exact correction by -+P: linear in L, see emu_rebuild_kernel), assembled
//                into 128 bits and rounded once to fp64 (two roundings in all: |fl(X) - X| <= 1 ulp), and C_ij -= X 2^-(sig_i + tau_j).
// alpha + beta is the largest integer with K 2^(alpha+beta) < P / 2 (P = p_1 .. p_L): the residues then determine X uniquely.  At L = 16
// (log2 P = 125.2) and K = 8192 that is alpha = 56, beta = 55: every row's largest entries are converted exactly, an entry 2^-e below its
// row's largest keeps 55 - e bits.  Each output row depends only on its own row of A and on B, whatever the tiling.
#include <math.h>
#include <stdint.h>
#include <stdlib.h>
#include <algorithm>

#include "common.h"

#include "gemm_tile.h"

typedef int v4i __attribute__((ext_vector_type(4)));
typedef int v16i __attribute__((ext_vector_type(16)));
typedef unsigned v4u __attribute__((ext_vector_type(4)));

#ifndef EMU_MFMA_16   // the product loop's MFMA shape, compile time only: 1 v_mfma_i32_16x16x64_i8, 0 v_mfma_i32_32x32x32_i8 (same LDS
#define EMU_MFMA_16 1 // image, staging, barriers and epilogue).  16 x 16 x 64 takes 8-11 % more cycles and holds a clock 13-18 % higher
#endif                // on random residues: 4-5 % less wall (profiles/r20_emu_product.txt; -DEMU_MFMA_16=0 repeats the A/B)

constexpr int EMU_MAXL = 16;
constexpr int EMU_BT = 256;   // int8 block tile: 256 x 256, 2 x 4 waves of 128 x 64 (4 x 2 MFMAs of 32 x 32), two waves per SIMD
constexpr int EMU_BK = 128;   // k bytes per LDS stage (one 128-byte row per operand row, the fp64 kernel's image geometry)

// pairwise coprime (256 = 2^8, 255 = 3 5 17, 253 = 11 23, 247 = 13 19, the rest prime); the first L are used
constexpr int EMU_MODULI[EMU_MAXL] = {256, 255, 253, 251, 247, 241, 239, 233, 229, 227, 223, 211, 199, 197, 193, 191};

static __constant__ const int emu_p[EMU_MAXL] = {256, 255, 253, 251, 247, 241, 239, 233, 229, 227, 223, 211, 199, 197, 193, 191};

// Chinese-remainder constants of the first L moduli (P = p_1 .. p_L, M_l = P / p_l): c[l] = M_l^-1 mod p_l, M_l and P cut into 40-bit
// limbs (M_l < 2^118: three, P < 2^126: four), 1 / P, and P / 2 and P as two 64-bit words.  One table per L, passed to the kernel by value.
typedef unsigned __int128 emu_u128;
struct EmuCrt {
    double m[EMU_MAXL][3], p[4], pinv;
    float c[EMU_MAXL];
    unsigned long p_lo, p_hi, half_lo, half_hi;
};
struct EmuCrtAll { EmuCrt t[EMU_MAXL + 1]; };   // t[L], L = 2 .. 16
constexpr EmuCrtAll emu_crt_tables()
{
    EmuCrtAll all{};
    constexpr emu_u128 mask = ((emu_u128)1 << 40) - 1;
    for (int L = 2; L <= EMU_MAXL; ++L) {
        EmuCrt &t = all.t[L];
        emu_u128 P = 1;
        for (int l = 0; l < L; ++l) P *= (emu_u128)EMU_MODULI[l];
        for (int l = 0; l < L; ++l) {
            const emu_u128 M = P / (emu_u128)EMU_MODULI[l];
            const int p = EMU_MODULI[l], a = (int)(M % (emu_u128)p);
            int inv = 0;
            for (int x = 1; x < p; ++x)
                if (a * x % p == 1) { inv = x; break; }
            t.c[l] = (float)inv;
            for (int j = 0; j < 3; ++j) t.m[l][j] = (double)(unsigned long)((M >> (40 * j)) & mask);
        }
        for (int j = 0; j < 4; ++j) t.p[j] = (double)(unsigned long)((P >> (40 * j)) & mask);
        t.pinv = 1.0 / (double)P;
        t.p_lo = (unsigned long)P;
        t.p_hi = (unsigned long)(P >> 64);
        t.half_lo = (unsigned long)(P >> 1);
        t.half_hi = (unsigned long)(P >> 65);
    }
    return all;
}
static constexpr EmuCrtAll emu_crt = emu_crt_tables();

#ifdef EMU_STAMP   // diagnostic build only (never the shipped library): s_memtime / s_memrealtime of every workgroup before its k loop,
// after it, and at kernel exit once its stores have landed: {cycles, 100 MHz} x {loop start, loop end, exit}
constexpr int EMU_STAMP_SLOTS = 1 << 16, EMU_STAMP_WIDTH = 6;
__device__ unsigned long emu_stamps[EMU_STAMP_SLOTS][EMU_STAMP_WIDTH];
extern "C" int gpx_emu_stamp_width() { return EMU_STAMP_WIDTH; }
extern "C" int gpx_emu_stamps(unsigned long *out, int n)
{
    return hipMemcpyFromSymbol(out, HIP_SYMBOL(emu_stamps), sizeof(unsigned long) * EMU_STAMP_WIDTH * std::min(n, EMU_STAMP_SLOTS)) == hipSuccess
               ? 0
               : GPX_ERR_HIP;
}
#endif

constexpr int EMU_NONFINITE = 0x7fffffff;   // row scale of a row that holds a NaN or an Inf: its outputs are NaN

// ---- switches (read once per process) -----------------------------------------------------------------------------
int emu_moduli()
{
    static const int v = [] { const char *e = getenv("GPX_EMU_MODULI"); const int l = e ? atoi(e) : EMU_MAXL; return std::min(EMU_MAXL, std::max(2, l)); }();
    return v;
}
static bool emu_k_ok(int64_t K) { return K > 0 && K % EMU_BK == 0 && K < (1 << 17); }   // the int8 k-stage; K 2^14 < 2^31 in the int32 accumulators
bool emu_enabled(int64_t K)
{
    static const int on = [] { const char *e = getenv("GPX_EMU_F64"); return e ? atoi(e) : 1; }();
    static const long min_k = [] { const char *e = getenv("GPX_EMU_MIN_K"); return e ? atol(e) : 4096L; }();
    return on && K >= min_k && emu_k_ok(K);
}
// alpha + beta: the largest integer s with K 2^s < P / 2
static int emu_scale_bits(int64_t K, int L)
{
    double log2p = 0.0;
    for (int l = 0; l < L; ++l) log2p += log2((double)EMU_MODULI[l]);
    return (int)floor(log2p - 1.0 - log2((double)K) - 1e-9);
}

// ---- residues of one integer, without a division or an fp64 reduction per modulus ------------------------------------------------------
// The integer a' (|a'| <= 2^59: emu_scale_bits(128, 16) = 117 gives abits = 59, the largest there is) is cut ONCE into two 32-bit words
// of a'' = a' + 2^60 = 2^32 hi + lo:  hi = floor(a' 2^-32) + 2^28 in [2^27, 3 2^27],  lo = a' - 2^32 floor(a' 2^-32) in [0, 2^32) (the
// fma is exact: lo is a multiple of a's ulp below 2^32).  The eight bytes d_0 .. d_7 of a'' (0 <= d_k <= 255, d_7 <= 0x18) are its limbs:
//   x = k0 + sum_k d_k (2^(8k) mod p),   k0 = (-2^60) mod p,   so x = a' (mod p),   0 <= x <= 254 + 8 255 254 < 2^19,
// two v_dot4_u32_u8 per modulus.  For odd p the symmetric residue is r = x - p q with q = floor((2 x + p) / (2 p)) (2 x + p is odd: no
// tie), and q = (y m) >> 32 for y = 2 x + p < 2^21, m = ceil(2^31 / p) < 2^24: y m / 2^32 exceeds y / (2 p) by less than 2^-11, and
// y / (2 p) lies at least 1 / (2 p) > 2^-9 below the next integer.  So |r| <= (p - 1) / 2 and the byte is r & 255.  Modulo 256 the byte
// is d_0 (the representative in [-128, 127]: +128 is stored as -128, the same residue).  tests/test_emulated_split_model.py walks every
// reachable x of every modulus through this arithmetic.
struct EmuSplitMod { unsigned c0, c1, k0, m; };
constexpr EmuSplitMod emu_split_mod(int l)
{
    const unsigned p = (unsigned)EMU_MODULI[l];
    EmuSplitMod t{};
    unsigned w = 1 % p;
    for (int k = 0; k < 8; ++k) {
        (k < 4 ? t.c0 : t.c1) |= w << (8 * (k & 3));
        w = w * 256 % p;
    }
    unsigned b = 1 % p;
    for (int i = 0; i < 60; ++i) b = 2 * b % p;
    t.k0 = (p - b) % p;
    t.m = (unsigned)((((unsigned long)1 << 31) + p - 1) / p);
    return t;
}
static_assert(EMU_MODULI[0] == 256, "the first modulus takes the low byte as it is");

// the two words of a'' for the integer a (|a| <= 2^59, exact in fp64)
static __device__ __forceinline__ void emu_words(double a, unsigned &lo, unsigned &hi)
{
    const double h = floor(a * 0x1p-32);
    lo = (unsigned)fma(-h, 0x1p32, a);
    hi = (unsigned)((int)h + (1 << 28));
}

// sixteen consecutive entries' residues modulo EMU_MODULI[l], one byte each, as the 16 bytes of plane l
template <int l> static __device__ __forceinline__ v4u emu_plane_bytes(const unsigned (&lo)[16], const unsigned (&hi)[16])
{
    int r[16];
    if constexpr (l == 0) {
#pragma unroll
        for (int e = 0; e < 16; ++e) r[e] = (int)lo[e];
    } else {
        constexpr EmuSplitMod M = emu_split_mod(l);
        constexpr int p = EMU_MODULI[l];
        static_assert(p % 2 == 1 && p < 256 && M.m < (1u << 24), "the reduction below is for odd moduli of one byte");
        // (the mask tells the compiler that the 24-bit multiply serves, and costs nothing; the multiply-add is named because the
        // compiler takes a 32-bit one, at a quarter of the rate; 256 q is added to r: only its low byte is kept)
        unsigned x[16], q[16];
#pragma unroll
        for (int e = 0; e < 16; ++e) x[e] = __builtin_amdgcn_udot4(lo[e], M.c0, M.k0, false);
#pragma unroll
        for (int e = 0; e < 16; ++e) x[e] = __builtin_amdgcn_udot4(hi[e], M.c1, x[e], false);
#pragma unroll
        for (int e = 0; e < 16; ++e) q[e] = __umulhi((2u * x[e] + (unsigned)p) & 0xffffffu, M.m);
#pragma unroll
        for (int e = 0; e < 16; ++e) asm("v_mad_u32_u24 %0, %1, %2, %3" : "=v"(r[e]) : "v"(q[e]), "s"(256 - p), "v"(x[e]));
    }
    v4u out;
#pragma unroll
    for (int g = 0; g < 4; ++g) {   // byte 0 of four words into one
        const unsigned w01 = __builtin_amdgcn_perm((unsigned)r[4 * g + 1], (unsigned)r[4 * g], 0x0c0c0400u);
        const unsigned w23 = __builtin_amdgcn_perm((unsigned)r[4 * g + 3], (unsigned)r[4 * g + 2], 0x0c0c0400u);
        out[g] = __builtin_amdgcn_perm(w23, w01, 0x05040100u);
    }
    return out;
}

template <int l> static __device__ __forceinline__ void emu_store_planes(const unsigned (&lo)[16], const unsigned (&hi)[16], int L,
                                                                         int8_t *__restrict__ out, long plane)
{
    if constexpr (l < EMU_MAXL) {
        if (l >= L) return;
        *reinterpret_cast<v4u *>(out) = emu_plane_bytes<l>(lo, hi);
        emu_store_planes<l + 1>(lo, hi, L, out + plane, plane);
    }
}

// ---- the split body: one lane takes 16 consecutive entries of a row (128 bytes of fp64 in, one 16-byte store per plane out), a wave a
// stretch of 1024 columns.  a' = rint(x 2^s).  zero (wave-uniform: a padding row, a row that holds a NaN or an Inf): zero residues,
// nothing is read.  CHECKED (the split with a given scale): a NaN or an Inf sets bad, an |a'| > lim sets over, either is stored as 0.
template <bool CHECKED>
static __device__ __forceinline__ void emu_split_lane(const double *__restrict__ x, bool zero, int s, double lim, int L, int8_t *__restrict__ out,
                                                      long plane, int &bad, int &over)
{
    if (zero) {
        for (int l = 0; l < L; ++l, out += plane) *reinterpret_cast<v4u *>(out) = (v4u){0u, 0u, 0u, 0u};
        return;
    }
    v2d v[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) v[j] = *reinterpret_cast<const v2d *>(x + 2 * j);
    unsigned lo[16], hi[16];
#pragma unroll
    for (int e = 0; e < 16; ++e) {
        const double xe = (e & 1) ? v[e >> 1].y : v[e >> 1].x;
        double a = rint(ldexp(xe, s));
        if (CHECKED) {
            const bool nf = !isfinite(xe), ok = fabs(a) <= lim;   // (a NaN or an Inf fails ok as well)
            bad |= (int)nf;
            over |= (int)(!ok && !nf);
            a = ok ? a : 0.0;
        }
        emu_words(a, lo[e], hi[e]);
    }
    emu_store_planes<0>(lo, hi, L, out, plane);
}

// ---- split: X [rows, K] (fp64, ldx) -> residue planes res[l][row][K] (int8) and the rows' scale exponents, in two launches ------------
// 1. one workgroup per row: the row's largest |x| gives sig[row] = bits - 1 - ilogb(max), so that |x| 2^sig < 2^bits for every entry (an
//    all-zero row and the padding rows keep 0), or EMU_NONFINITE where the row holds a NaN or an Inf;
// 2. one wave per (row, stretch of 1024 columns): the split body; nothing can exceed 2^bits, a padding or a non-finite row is zero.
__global__ __launch_bounds__(256) void emu_row_scale_kernel(const double *__restrict__ X, long ldx, long rows_real, int K, int bits,
                                                            int *__restrict__ sig)
{
    const long row = blockIdx.x;
    const int t = threadIdx.x;
    if (row >= rows_real) {
        if (t == 0) sig[row] = 0;
        return;
    }
    __shared__ double red_max[4];
    __shared__ int red_bad[4];
    const double *x = X + row * ldx;
    double m = 0.0;
    int bad = 0;
#pragma unroll 4
    for (int c = 2 * t; c < K; c += 512) {
        const v2d v = *reinterpret_cast<const v2d *>(x + c);
        bad |= (int)!isfinite(v.x) | (int)!isfinite(v.y);
        m = fmax(m, fmax(fabs(v.x), fabs(v.y)));
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) { m = fmax(m, __shfl_xor(m, o)); bad |= __shfl_xor(bad, o); }
    if ((t & 63) == 0) { red_max[t >> 6] = m; red_bad[t >> 6] = bad; }
    __syncthreads();
    if (t == 0) {
        m = fmax(fmax(red_max[0], red_max[1]), fmax(red_max[2], red_max[3]));
        bad = red_bad[0] | red_bad[1] | red_bad[2] | red_bad[3];
        sig[row] = bad ? EMU_NONFINITE : (m == 0.0 ? 0 : bits - 1 - ilogb(m));
    }
}

__global__ __launch_bounds__(256) void emu_split_kernel(const double *__restrict__ X, long ldx, long rows_real, long rows_pad, int K, int L,
                                                        int8_t *__restrict__ res, long plane, const int *__restrict__ sig)
{
    const int stretches = (K + 1023) >> 10;
    const long item = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
    const long row = item / stretches;
    const int c = (int)(item - row * stretches) * 1024 + 16 * (threadIdx.x & 63);
    if (row >= rows_pad || c >= K) return;
    const int s = row < rows_real ? sig[row] : EMU_NONFINITE;
    int bad = 0, over = 0;
    emu_split_lane<false>(X + row * ldx + c, s == EMU_NONFINITE, s, 0.0, L, res + row * (long)K + c, plane, bad, over);
}

// ---- split with a given scale (the left-looking solve, tsolve.hip): the rows of one solved slab of `width` columns (a multiple of 16,
// at most 1024: one wave per row) into the persistent residue image res[l][row][ldr] at the slab's column offset, with the scale sig[row]
// that emu_scale_from_bound_kernel derived from the row's bound before the row was known.  An entry with |x 2^s| > 2^bits (the bound was
// wrong) raises *status and is stored as 0: it never wraps silently; a NaN or an Inf marks the row (sig = EMU_NONFINITE, sticky: every
// later product of the row is NaN) and raises nothing.  Rows >= rows_real (padding) and rows marked at entry are zero.
__global__ __launch_bounds__(256) void emu_split_fixed_kernel(const double *__restrict__ X, long ldx, long rows_real, long rows_pad, int width,
                                                              int bits, int L, int8_t *__restrict__ res, long ldr, long plane, int *sig, int *status)
{
    const long row = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
    const int lane = threadIdx.x & 63, c = 16 * lane;
    if (row >= rows_pad) return;
    const int s = row < rows_real ? sig[row] : EMU_NONFINITE;
    const bool dead = s == EMU_NONFINITE;
    int bad = 0, over = 0;
    if (c < width) emu_split_lane<true>(X + row * ldx + c, dead, s, ldexp(1.0, bits), L, res + row * ldr + c, plane, bad, over);
    if (dead) return;
    bad = __any(bad);
    over = __any(over);
    if (lane == 0) {
        if (bad) sig[row] = EMU_NONFINITE;
        else if (over) atomicMax(status, 1);
    }
}

// sig[i] = bits - 1 - ilogb(2 bound_i): |x| <= bound_i scales below 2^(bits - 1), one bit of headroom for the rounding of the solve that
// the bound was derived without.  bound 0 (padding rows, an all-zero row): a scale at which every double of magnitude 2^(bits - 1000) or
// more exceeds 2^bits and raises *status; a smaller non-zero one (down to about 2^-1000, below which x 2^1000 rounds to 0 unseen) is held
// exactly or rounded to an integer, which is harmless next to a bound of 0.  A bound that is negative, NaN or Inf is no bound: *status is
// raised and the caller takes the other route.
constexpr int EMU_ZERO_BOUND_SCALE = 1000;
__global__ __launch_bounds__(256) void emu_scale_from_bound_kernel(const double *__restrict__ bound, long rows, long rows_pad, int bits,
                                                                   int *__restrict__ sig, int *status)
{
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= rows_pad) return;
    const double b = i < rows ? bound[i] : 0.0;
    int s = 0;
    if (!(b >= 0.0) || isinf(b)) atomicMax(status, 1);
    else s = b == 0.0 ? EMU_ZERO_BOUND_SCALE : bits - 2 - ilogb(b);
    sig[i] = s;
}

// ---- products: R_l = (A_l B_l^T) mod p_l, int8 in, int32 accumulate, one byte out -----------------------------------------------------
// One launch covers every modulus: workgroup -> (l, by, bx) in an XCD-aware order (each XCD takes a contiguous chunk of the logical order;
// inside a modulus groups of 8 tile rows, column-major, so the tiles resident on an XCD share A and B panels through its L2).
// LDS image, staging and swizzle as gemm_tile.h: per stage [256][128 B] of A then of B, filled by LDS-DMA (16 B per lane, 8 rows per
// wave-instruction), granule index XOR (row >> 1) & 7 on the source address and on the fragment reads; a 32 x 32 x 32 fragment is one
// ds_read_b128 per lane (row lane & 31, k-bytes 16 (lane >> 5) .. +15 of a 32-byte slice), conflict-free under that swizzle.
// A, B: planes of [tm 256][lda] and [tn 256][K] bytes (B packed: ldb = K; lda >= K is the row stride of A's planes, so that a product
// reads columns 0 .. K of a wider residue image: a panel's byte offsets stay below 256 lda < 2^25, its 64-bit base comes from the
// host's row tile and from z, by); R: planes of [tm 256][ldr] bytes.
//
// EMU_MFMA_16: the wave tile (128 x 64) as 8 x 4 MFMAs of 16 x 16 x 64.  A fragment is one ds_read_b128 per lane: row fr = lane & 15 of a
// 16-row tile, k-bytes 16 fq .. +15 (fq = lane >> 4) of the 64-byte slice kk, at granule (4 kk + fq) ^ ((fr >> 1) & 7) of its 128-byte
// row.  Banks are (a / 4) % 64: a 256-byte bank row holds LDS rows 2n and 2n + 1, so a lane's 16-byte slot is 8 (fr & 1) + granule.
// ds_read_b128 is served in the lane groups {0-3, 12-15, 20-27}, {4-11, 16-19, 28-31} and the same + 32.  The first holds rows 0-3 and
// 12-15 at fq = 0 and rows 4-11 at fq = 1: of either parity that is fr >> 1 in {0, 1, 6, 7} at granule c ^ (fr >> 1) and fr >> 1 in
// {2, 3, 4, 5} at granule c ^ 1 ^ (fr >> 1) (c = 4 kk): c ^ {0, 1, 6, 7, 3, 2, 5, 4}, eight distinct granules per parity, sixteen distinct
// slots.  The second group swaps the two fq, the other two XOR every granule with 2: all conflict-free, as the 32-row read is.
//
// Epilogue (either shape): registers 4 g .. 4 g + 3 of an accumulator are four consecutive rows of one column; |v| < 2^31 is exact in fp64
// and v / p is never within 1 / (2p) of a half-integer for odd p (256: a tie wraps to the same byte).  One byte store per residue: the
// stores cost nothing that shows (profiles/r20_emu_product.txt, which also has the integer reduction and the 16-byte stores through an
// LDS image that were tried in their place: tools/native/rejected/r20_emu_epilogue_int_wide.patch).
__global__ __launch_bounds__(512, 1) void emu_i8_gemm_kernel(const int8_t *__restrict__ A, const int8_t *__restrict__ B, long sa, long sb, int K,
                                                             int8_t *__restrict__ R, long ldr, long sr, int tm, int tn, int lda)
{
    __shared__ __attribute__((aligned(1024))) int8_t smem[2 * 2 * EMU_BT * EMU_BK];   // 128 KiB: two stages of A and B
    constexpr int STAGE = 2 * EMU_BT * EMU_BK;
    const int nwg = gridDim.x, orig = blockIdx.x;
    const int lid = xcd_chunk_start(nwg, orig & 7) + (orig >> 3);
    const int per = tm * tn, z = lid / per;
    int rem = lid - z * per;
    const int g = rem / (8 * tn), first = 8 * g, grows = std::min(8, tm - first);
    rem -= g * 8 * tn;
    const int bx = rem / grows, by = first + rem - bx * grows;

    const int t = threadIdx.x;
    const int wave = __builtin_amdgcn_readfirstlane(t >> 6), lane = t & 63;
    const int wr = wave >> 2, wc = wave & 3;
    const int drow = lane >> 3;
    const char *Abase = reinterpret_cast<const char *>(A + z * sa + (long)by * EMU_BT * lda);
    const char *Bbase = reinterpret_cast<const char *>(B + z * sb + (long)bx * EMU_BT * K);
    unsigned offa[4], offb[4];   // instruction u of this wave covers rows 8 (wave + 8 u) .. +7 of either operand's 256-row panel
#pragma unroll
    for (int u = 0; u < 4; ++u) {
        const int row = 8 * (wave + 8 * u) + drow;
        offa[u] = (unsigned)((long)row * lda + 16 * ((lane & 7) ^ ((row >> 1) & 7)));
        offb[u] = (unsigned)((long)row * K + 16 * ((lane & 7) ^ ((row >> 1) & 7)));
    }
    const unsigned lds_base = (unsigned)(unsigned long)(__attribute__((address_space(3))) int8_t *)smem;
#define EMU_DMA_ONE(SBASE, VOFF, LDSBYTES) \
    asm volatile("s_mov_b32 m0, %0\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %1, %2" ::"s"(LDSBYTES), "v"(VOFF), "s"(SBASE) : "memory");
#define EMU_DMA_STAGE(BUF, KT)                                                                                              \
    {                                                                                                                       \
        const char *ak_ = gpx_uniform_ptr(Abase + (long)(KT) * EMU_BK);                                                     \
        const char *bk_ = gpx_uniform_ptr(Bbase + (long)(KT) * EMU_BK);                                                     \
        _Pragma("unroll") for (int u_ = 0; u_ < 4; ++u_)                                                                    \
            EMU_DMA_ONE(ak_, offa[u_], __builtin_amdgcn_readfirstlane(lds_base + (unsigned)((BUF) * STAGE + (wave + 8 * u_) * 1024)))  \
        _Pragma("unroll") for (int u_ = 0; u_ < 4; ++u_)                                                                    \
            EMU_DMA_ONE(bk_, offb[u_], __builtin_amdgcn_readfirstlane(lds_base + (unsigned)((BUF) * STAGE + EMU_BT * EMU_BK + (wave + 8 * u_) * 1024))) \
    }
    const int nk = K / EMU_BK;
    EMU_DMA_STAGE(0, 0)
#if EMU_MFMA_16
    v4i acc[8][4];
#pragma unroll
    for (int i = 0; i < 8; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[i][j] = (v4i){};
#else
    v16i acc[4][2];
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j) acc[i][j] = (v16i){};
#endif
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
#ifdef EMU_STAMP
    const unsigned long stamp_c0 = __builtin_amdgcn_s_memtime(), stamp_r0 = __builtin_amdgcn_s_memrealtime();
#endif

    typedef const __attribute__((address_space(3))) v4i lds_v4i;
    const __attribute__((address_space(3))) int8_t *lsm = (const __attribute__((address_space(3))) int8_t *)smem;
#if EMU_MFMA_16
    // a stage is four sub-steps (slice kk, half h of the wave's eight A tiles) of 4 x 4 MFMAs: the A fragments alternate between two sets
    // per sub-step, the B fragments per kk, so the loads of a sub-step ride under the MFMAs of the one before, as in the 32 x 32 x 32 loop
    const int fr = lane & 15, fq = lane >> 4, sw = (fr >> 1) & 7;
    int koff[2];
#pragma unroll
    for (int kk = 0; kk < 2; ++kk) koff[kk] = 16 * ((4 * kk + fq) ^ sw);
    const int a_row = (wr * 128 + fr) * EMU_BK, b_row = EMU_BT * EMU_BK + (wc * 64 + fr) * EMU_BK;
    v4i fa[2][4], fb[2][4];
#define EMU_LOAD_A(SET, BUFOFF, KK, H)                                                               \
    _Pragma("unroll") for (int i_ = 0; i_ < 4; ++i_)                                                 \
        fa[SET][i_] = *(lds_v4i *)(lsm + (BUFOFF) + a_row + (4 * (H) + i_) * 16 * EMU_BK + koff[KK]);
#define EMU_LOAD_B(SET, BUFOFF, KK)                                                                  \
    _Pragma("unroll") for (int j_ = 0; j_ < 4; ++j_)                                                 \
        fb[SET][j_] = *(lds_v4i *)(lsm + (BUFOFF) + b_row + j_ * 16 * EMU_BK + koff[KK]);
#define EMU_MMA(ASET, BSET, H)                                                                       \
    _Pragma("unroll") for (int i_ = 0; i_ < 4; ++i_)                                                 \
        _Pragma("unroll") for (int j_ = 0; j_ < 4; ++j_)                                             \
            acc[4 * (H) + i_][j_] = __builtin_amdgcn_mfma_i32_16x16x64_i8(fa[ASET][i_], fb[BSET][j_], acc[4 * (H) + i_][j_], 0, 0, 0);
    EMU_LOAD_A(0, 0, 0, 0)
    EMU_LOAD_B(0, 0, 0)
#define EMU_KSTEP(CUR_OFF, NXT_OFF, NXT_BUF, KT)                   \
    {                                                             \
        const bool has_next_ = (KT) + 1 < nk;                     \
        if (has_next_) EMU_DMA_STAGE(NXT_BUF, (KT) + 1)           \
        EMU_LOAD_A(1, CUR_OFF, 0, 1)                              \
        EMU_MMA(0, 0, 0)                                          \
        __builtin_amdgcn_sched_barrier(0);                        \
        EMU_LOAD_A(0, CUR_OFF, 1, 0)                              \
        EMU_LOAD_B(1, CUR_OFF, 1)                                 \
        EMU_MMA(1, 0, 1)                                          \
        __builtin_amdgcn_sched_barrier(0);                        \
        EMU_LOAD_A(1, CUR_OFF, 1, 1)                              \
        EMU_MMA(0, 1, 0)                                          \
        __builtin_amdgcn_sched_barrier(0);                        \
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");          \
        __syncthreads();                                          \
        if (has_next_) { EMU_LOAD_A(0, NXT_OFF, 0, 0) EMU_LOAD_B(0, NXT_OFF, 0) } \
        EMU_MMA(1, 1, 1)                                          \
        __builtin_amdgcn_sched_barrier(0);                        \
    }
    for (int kt = 0; kt < nk; kt += 2) {
        EMU_KSTEP(0, STAGE, 1, kt)
        if (kt + 1 < nk) EMU_KSTEP(STAGE, 0, 0, kt + 1)
    }
#undef EMU_KSTEP
#undef EMU_LOAD_A
#undef EMU_LOAD_B
#undef EMU_MMA
#else
    const int fr = lane & 31, sw = (fr >> 1) & 7;
    int koff[4];
#pragma unroll
    for (int kk = 0; kk < 4; ++kk) koff[kk] = 16 * ((2 * kk + (lane >> 5)) ^ sw);
    const int a_row = (wr * 128 + fr) * EMU_BK, b_row = EMU_BT * EMU_BK + (wc * 64 + fr) * EMU_BK;
    v4i fa[2][4], fb[2][2];
#define EMU_LOAD_FRAGS(SET, BUFOFF, KK)                                                              \
    _Pragma("unroll") for (int i_ = 0; i_ < 4; ++i_)                                                 \
        fa[SET][i_] = *(lds_v4i *)(lsm + (BUFOFF) + a_row + i_ * 32 * EMU_BK + koff[KK]);            \
    _Pragma("unroll") for (int i_ = 0; i_ < 2; ++i_)                                                 \
        fb[SET][i_] = *(lds_v4i *)(lsm + (BUFOFF) + b_row + i_ * 32 * EMU_BK + koff[KK]);
#define EMU_MMA(SET)                                                                                 \
    _Pragma("unroll") for (int i_ = 0; i_ < 4; ++i_)                                                 \
        _Pragma("unroll") for (int j_ = 0; j_ < 2; ++j_)                                             \
            acc[i_][j_] = __builtin_amdgcn_mfma_i32_32x32x32_i8(fa[SET][i_], fb[SET][j_], acc[i_][j_], 0, 0, 0);
    EMU_LOAD_FRAGS(0, 0, 0)
#define EMU_KSTEP(CUR_OFF, NXT_OFF, NXT_BUF, KT)                   \
    {                                                             \
        const bool has_next_ = (KT) + 1 < nk;                     \
        if (has_next_) EMU_DMA_STAGE(NXT_BUF, (KT) + 1)           \
        EMU_LOAD_FRAGS(1, CUR_OFF, 1)                             \
        EMU_MMA(0)                                                \
        __builtin_amdgcn_sched_barrier(0);                        \
        EMU_LOAD_FRAGS(0, CUR_OFF, 2)                             \
        EMU_MMA(1)                                                \
        __builtin_amdgcn_sched_barrier(0);                        \
        EMU_LOAD_FRAGS(1, CUR_OFF, 3)                             \
        EMU_MMA(0)                                                \
        __builtin_amdgcn_sched_barrier(0);                        \
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");          \
        __syncthreads();                                          \
        if (has_next_) { EMU_LOAD_FRAGS(0, NXT_OFF, 0) }          \
        EMU_MMA(1)                                                \
        __builtin_amdgcn_sched_barrier(0);                        \
    }
    for (int kt = 0; kt < nk; kt += 2) {
        EMU_KSTEP(0, STAGE, 1, kt)
        if (kt + 1 < nk) EMU_KSTEP(STAGE, 0, 0, kt + 1)
    }
#undef EMU_KSTEP
#undef EMU_LOAD_FRAGS
#undef EMU_MMA
#endif
#undef EMU_DMA_STAGE
#undef EMU_DMA_ONE
#ifdef EMU_STAMP
    const unsigned long stamp_c1 = __builtin_amdgcn_s_memtime(), stamp_r1 = __builtin_amdgcn_s_memrealtime();
#endif

    // epilogue
#if EMU_MFMA_16
    constexpr int TI = 8, TJ = 4, TG = 1, TW = 16;   // accumulator register r of tile (i, j): row 16 i + 4 fq + r, column 16 j + fr
    const int row0 = 4 * fq;
#else
    constexpr int TI = 4, TJ = 2, TG = 4, TW = 32;   // row 32 i + 8 (r >> 2) + 4 (lane >> 5) + (r & 3), column 32 j + fr
    const int row0 = 4 * (lane >> 5);
#endif
    const double p = (double)emu_p[z], pinv = 1.0 / p;
    int8_t *Rw = R + z * sr + ((long)by * EMU_BT + wr * 128 + row0) * ldr + (long)bx * EMU_BT + wc * 64 + fr;
#pragma unroll
    for (int i = 0; i < TI; ++i)
#pragma unroll
        for (int j = 0; j < TJ; ++j)
#pragma unroll
            for (int g = 0; g < TG; ++g)
#pragma unroll
                for (int b = 0; b < 4; ++b) {
                    const double v = (double)acc[i][j][4 * g + b];
                    Rw[(long)(i * TW + 8 * g + b) * ldr + j * TW] = (int8_t)(int)fma(-rint(v * pinv), p, v);
                }
#ifdef EMU_STAMP
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    if (t == 0 && orig < EMU_STAMP_SLOTS) {
        unsigned long *st = emu_stamps[orig];
        st[0] = stamp_c0; st[1] = stamp_c1; st[2] = stamp_r0; st[3] = stamp_r1;
        st[4] = __builtin_amdgcn_s_memtime(); st[5] = __builtin_amdgcn_s_memrealtime();
    }
#endif
}

// ---- rebuild: C_ij -= X_ij 2^-(sig_i + tau_j), four consecutive columns per thread ----------------------------------------------
constexpr long EMU_NO_DIAG = 1L << 40;   // `diag` of a full rectangle
// X is the integer in [-P/2, P/2) with the L residues r_l, by the direct CRT sum (linear in L):
//   t_l = r_l c_l mod p_l, any representative with |t_l| <= (p_l + 1) / 2 (|r_l c_l| < 2^15: exact in fp32, one step per modulus);
//   S = sum_l t_l M_l = X (mod P), summed limb by limb in fp64 (|t_l| <= 128 and limbs below 2^40: every partial sum is an integer
//   below 2^51, so the 3 L FMAs are exact);  q = rint(S / P) from the fp64 value of S (|q| <= 8, off by one at most, and only when
//   S / P is within 2^-40 of a half-integer);  X = S - q P limb by limb (exact), assembled into 128 bits;  one exact correction by
//   -+P where X fell outside [-P/2, P/2) makes q's rounding immaterial.  The integer is rounded once to fp64, as before.
__global__ __launch_bounds__(256) void emu_rebuild_kernel(const int8_t *__restrict__ R, long ldr, long sr, int L, const EmuCrt T,
                                                          const int *__restrict__ sa, const int *__restrict__ sb, double *__restrict__ C,
                                                          long ldc, long rows, long cols, long diag, long dmask)
{
    const long q4 = (cols + 3) >> 2;
    const long idx = (long)blockIdx.x * 256 + threadIdx.x;
    const long i = idx / q4, j0 = (idx - i * q4) * 4;
    if (i >= rows) return;
    unsigned w[EMU_MAXL];
#pragma unroll
    for (int l = 0; l < EMU_MAXL; ++l)
        w[l] = l < L ? *reinterpret_cast<const unsigned *>(R + l * sr + i * ldr + j0) : 0u;   // (the table of L is zero from l = L on)
    const int si = sa[i];
    double *c = C + i * ldc + j0;
    const __int128 P = (__int128)(((emu_u128)T.p_hi << 64) | T.p_lo), half = (__int128)(((emu_u128)T.half_hi << 64) | T.half_lo);
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        if (j0 + e >= cols || j0 + e > ((i + diag) | dmask)) continue;   // (row i ends at column (i + diag) | dmask -- EMU_NO_DIAG: at cols)
        const int tj = sb[j0 + e];
        if (si == EMU_NONFINITE || tj == EMU_NONFINITE) { c[e] = __builtin_nan(""); continue; }
        double s0 = 0.0, s1 = 0.0, s2 = 0.0;
#pragma unroll
        for (int l = 0; l < EMU_MAXL; ++l) {
            const float pl = (float)emu_p[l], plinv = 1.0f / pl;
            float t = (float)(int8_t)(w[l] >> (8 * e)) * T.c[l];
            t = fmaf(-rintf(t * plinv), pl, t);
            const double td = (double)t;
            s0 = fma(td, T.m[l][0], s0);
            s1 = fma(td, T.m[l][1], s1);
            s2 = fma(td, T.m[l][2], s2);
        }
        const double q = rint(fma(fma(s2, 0x1p40, s1), 0x1p40, s0) * T.pinv);
        const long x0 = (long)fma(-q, T.p[0], s0), x1 = (long)fma(-q, T.p[1], s1), x2 = (long)fma(-q, T.p[2], s2), x3 = (long)(-q * T.p[3]);
        // the sum is below 3 P / 2 < 2^127 in magnitude; its terms are not, so they are added modulo 2^128
        __int128 X = (__int128)((emu_u128)(__int128)x0 + ((emu_u128)(__int128)x1 << 40) + ((emu_u128)(__int128)x2 << 80) + ((emu_u128)(__int128)x3 << 120));
        X = X >= half ? X - P : (X < -half ? X + P : X);
        const long hi = (long)(X >> 64);
        const unsigned long lo = (unsigned long)X;
        const double xd = (hi == ((long)lo >> 63)) ? (double)(long)lo : fma((double)hi, 0x1p64, (double)lo);
        c[e] -= ldexp(xd, -(si + tj));
    }
}

// the two launches of the split with its own scale, and the one of the split with a given scale
static void emu_launch_split(const double *X, long ldx, long rows, long rows_pad, int K, int bits, int L, int8_t *res, long plane, int *sig,
                             hipStream_t s)
{
    const long waves = rows_pad * ((K + 1023) / 1024);
    hipLaunchKernelGGL(emu_row_scale_kernel, dim3((unsigned)rows_pad), dim3(256), 0, s, X, ldx, rows, K, bits, sig);
    hipLaunchKernelGGL(emu_split_kernel, dim3((unsigned)((waves + 3) / 4)), dim3(256), 0, s, X, ldx, rows, rows_pad, K, L, res, plane, (const int *)sig);
}
static void emu_launch_split_fixed(const double *X, long ldx, long rows, long rows_pad, int width, int bits, int L, int8_t *res, long ldr, long plane,
                                   int *sig, int *status, hipStream_t s)
{
    hipLaunchKernelGGL(emu_split_fixed_kernel, dim3((unsigned)((rows_pad + 3) / 4)), dim3(256), 0, s, X, ldx, rows, rows_pad, width, bits, L, res, ldr,
                       plane, sig, status);
}

// ---- workspace -------------------------------------------------------------------------------------------------------------
// One frame for the three drivers below (common.h: EmuFrame).  Residues of a row tile of A, of a column tile of B and the product residues
// of their block, each at most 2 GiB: at N = M = 16384 (K = 8192) one tile of each; deeper products (K = 32768 at N = 65536) loop over row
// tiles and, inside, column tiles.  Every need grows with rows, so a workspace reserved for a predict chunk serves every shorter chunk.
static int64_t emu_cap(int64_t K, int L) { return std::max<int64_t>(EMU_BT, (((int64_t)1 << 31) / (K * L)) / EMU_BT * EMU_BT); }

void EmuFrame::reserve(const EmuPlan &p)
{
    held = {std::max(held.img, p.need.img), std::max(held.b, p.need.b), std::max(held.r, p.need.r), std::max(held.sig, p.need.sig),
            std::max(held.bound, p.need.bound)};
}

// n blocks from the pool (an empty one is skipped) or none: after a refusal what was taken has gone back at once (nothing is queued on it)
static int emu_take(double **q, const int64_t *bytes, int n, Scratch *sc)
{
    int rc = 0;
    for (int i = 0; i < n; ++i) q[i] = nullptr;
    for (int i = 0; i < n && !rc; ++i)
        if (bytes[i]) rc = dalloc(&q[i], (bytes[i] + 7) / 8);
    for (int i = 0; i < n; ++i)
        if (q[i] && rc) { dfree(q[i]); q[i] = nullptr; }
        else if (q[i] && sc) sc->blocks.push_back(q[i]);
    return rc;
}

int emu_alloc(EmuFrame &w, Scratch *sc)
{
    double *q[5];
    const int64_t bytes[5] = {w.held.img, w.held.b, w.held.r, w.held.sig * (int64_t)sizeof(int), w.held.bound * (int64_t)sizeof(double)};
    const int rc = emu_take(q, bytes, 5, sc);   // no room: the caller keeps its other route
    w.a.base = (int8_t *)q[0]; w.rb = (int8_t *)q[1]; w.rr = (int8_t *)q[2];
    w.sig = (int *)q[3]; w.bound = q[4];
    return rc;
}

void emu_free(EmuFrame &w)
{
    for (void *p : {(void *)w.a.base, (void *)w.rb, (void *)w.rr, (void *)w.sig, (void *)w.bound}) dfree(p);
    w.a.base = w.rb = w.rr = nullptr; w.sig = nullptr; w.bound = nullptr;
}

// the blocks held cover plan p (the frame's own, or the recursion's plan of one product) and the product residues of a full tile pair
static int emu_fits(const EmuFrame &w, const EmuPlan &p, const char *what)
{
    const EmuNeed &h = w.held, &n = p.need;
    if (w.a.base && n.img <= h.img && n.b <= h.b && n.r <= h.r && p.a.rt * p.ct * p.a.L <= h.r && n.sig <= h.sig && n.bound <= h.bound) return 0;
    gpx_set_error("%s: workspace too small for %ld rows x K = %ld", what, (long)p.a.rows_pad, (long)p.a.ld);
    return GPX_ERR_STATE;
}

// a plan's first fields: L moduli, rows of ld bytes, the scale bits of a product of depth ld (halves: bits / 2 in either role)
static EmuPlan emu_plan_begin(int64_t ld, bool halves)
{
    EmuPlan p;
    p.a.L = emu_moduli();
    p.a.ld = ld;
    p.bbits = emu_scale_bits(ld, (int)p.a.L) / 2;
    p.abits = halves ? p.bbits : emu_scale_bits(ld, (int)p.a.L) - p.bbits;
    return p;
}

// ---- the tile step: what every driver does for one (row tile, column tile) pair ----------------------------------------------------
// R_l = (A_l B_l^T) mod p_l over tm x tn blocks of 256 x 256, R as planes of [256 tm][ldr] bytes sr apart; what emu_i8_gemm_kernel takes
// for granted (its comment) is checked here, once for every caller
static int emu_launch_product(const EmuOperand &a, const EmuOperand &b, int8_t *R, int64_t ldr, int64_t sr, int64_t tm, int64_t tn, int64_t K, int L,
                              hipStream_t s)
{
    const int64_t lim = (int64_t)1 << 31;
    if (!emu_k_ok(K) || b.ld != K || a.ld < K || L * a.plane > lim || L * b.plane > lim || (EMU_BT - 1) * a.ld + K >= lim || tm * tn * L > INT32_MAX) {
        gpx_set_error("emu: int8 product of %ld x %ld blocks, K = %ld, row stride %ld, %d moduli outside the kernel's range", (long)tm, (long)tn, (long)K, (long)a.ld, L);
        return GPX_ERR_STATE;
    }
    hipLaunchKernelGGL(emu_i8_gemm_kernel, dim3((unsigned)(tm * tn * L)), dim3(512), 0, s, a.res, b.res, (long)a.plane, (long)b.plane, (int)K, R, (long)ldr,
                       (long)sr, (int)tm, (int)tn, (int)a.ld);
    return 0;
}

static void emu_launch_rebuild(const int8_t *R, int64_t ldr, int64_t sr, int L, const int *sa, const int *sb, double *C, int64_t ldc, int64_t rows,
                               int64_t cols, int64_t diag, int64_t dmask, hipStream_t s)
{
    const long thr = (long)rows * ((cols + 3) / 4);
    hipLaunchKernelGGL(emu_rebuild_kernel, dim3((unsigned)((thr + 255) / 256)), dim3(256), 0, s, R, (long)ldr, (long)sr, L, emu_crt.t[L], sa, sb, C, (long)ldc,
                       (long)rows, (long)cols, (long)diag, (long)dmask);
}

// C[nr, nc] -= A B^T for nr rows of a (nrp: padded to 256, the rows of residues) and nc of b (ncp), through rr as planes of [nrp][ncp];
// row i of C ends at column (i + diag) | dmask (EMU_NO_DIAG, 0: the full rectangle)
static int emu_tile_update(const EmuOperand &a, const EmuOperand &b, int8_t *rr, double *C, int64_t ldc, int64_t nr, int64_t nrp, int64_t nc, int64_t ncp,
                           int64_t K, int L, int64_t diag, int64_t dmask, hipStream_t s)
{
    GPX_TRY(emu_launch_product(a, b, rr, ncp, nrp * ncp, nrp / EMU_BT, ncp / EMU_BT, K, L, s));
    emu_launch_rebuild(rr, ncp, nrp * ncp, L, a.scale, b.scale, C, ldc, nr, nc, diag, dmask, s);
    return 0;
}

// What the kernels take for granted of a caller outside the library (gpx_emu_gemm_nt_sub; tsolve.hip passes slabs of 128-padded matrices at
// offsets that are multiples of 1024), checked on the host before anything is allocated or queued: K a multiple of 128 below 2^17 (the
// int8 k-stage; K 2^14 < 2^31 in the int32 accumulators), leading dimensions that hold a row (lda, ldb >= K, ldc >= cols), and rows of
// A and B that start on 16 bytes (base pointers 16-byte aligned, lda and ldb even): the split kernels read pairs of doubles.
static int emu_check_args(const double *A, int64_t lda, const double *B, int64_t ldb, int64_t ldc, int64_t cols, int64_t K)
{
    if (!emu_k_ok(K)) {
        gpx_set_error("emu_gemm_nt_sub: K = %ld is not a multiple of %d in [%d, 2^17)", (long)K, EMU_BK, EMU_BK);
        return GPX_ERR_BAD_ARG;
    }
    if (lda < K || ldb < K || ldc < cols) {
        gpx_set_error("emu_gemm_nt_sub: leading dimension shorter than a row (lda %ld, ldb %ld < K %ld, or ldc %ld < cols %ld)", (long)lda, (long)ldb,
                      (long)K, (long)ldc, (long)cols);
        return GPX_ERR_BAD_ARG;
    }
    if ((lda | ldb) & 1 || ((uintptr_t)A | (uintptr_t)B) & 15) {
        gpx_set_error("emu_gemm_nt_sub: A and B must be 16-byte aligned with even lda, ldb (lda %ld, ldb %ld, A %p, B %p)", (long)lda, (long)ldb,
                      (const void *)A, (const void *)B);
        return GPX_ERR_BAD_ARG;
    }
    return 0;
}

// ---- C[rows, cols] -= A[rows, K] B[cols, K]^T (row-major, fp64), in a workspace that holds emu_work_plan of at least these shapes ---------
// Row tiles of `cap` rows with a ragged last one, each split into the image's one tile; B's column tile shrunk while a tile pair's
// product residues would pass 2 GiB (its block and scales stay sized for the unshrunk tile).  bits - bits / 2 for A, bits / 2 for B.
EmuPlan emu_work_plan(int64_t rows, int64_t cols, int64_t K)
{
    EmuPlan p = emu_plan_begin(K, false);
    const int64_t L = p.a.L, cap = emu_cap(K, (int)L);
    p.a.tiles = 1;
    p.a.rt = p.a.rows_pad = std::min(round_up(rows, EMU_BT), cap);
    p.ct = std::min(round_up(cols, EMU_BT), cap);
    p.need = {p.a.rt * K * L, p.ct * K * L, std::min(p.a.rt * p.ct * L, (int64_t)1 << 31), p.a.rt + p.ct, 0};
    while (p.ct > EMU_BT && p.a.rt * p.ct * L > ((int64_t)1 << 31)) p.ct -= EMU_BT;
    return p;
}

int emu_gemm_nt_sub(const double *A, int64_t lda, const double *B, int64_t ldb, double *C, int64_t ldc, int64_t rows, int64_t cols, int64_t K,
                    const EmuFrame &w, hipStream_t s, Profiler *prof)
{
    if (rows <= 0 || cols <= 0) return 0;
    if (!emu_k_ok(K)) { gpx_set_error("emu_gemm_nt_sub: K = %ld out of range", (long)K); return GPX_ERR_BAD_ARG; }
    const EmuPlan p = emu_work_plan(rows, cols, K);
    GPX_TRY(emu_fits(w, p, "emu_gemm_nt_sub"));
    ProfScope ps(prof, s, GPX_K_GEMM_EMU, 2.0 * (double)rows * (double)cols * (double)K);
    const int L = (int)p.a.L;
    int *sga = w.sig, *sgb = sga + p.a.rt;
    for (int64_t r0 = 0; r0 < rows; r0 += p.a.rt) {
        const int64_t nr = std::min(p.a.rt, rows - r0), nrp = round_up(nr, EMU_BT);
        emu_launch_split(A + r0 * lda, (long)lda, (long)nr, (long)nrp, (int)K, p.abits, L, w.a.base, (long)(nrp * K), sga, s);
        for (int64_t c0 = 0; c0 < cols; c0 += p.ct) {
            const int64_t nc = std::min(p.ct, cols - c0), ncp = round_up(nc, EMU_BT);
            emu_launch_split(B + c0 * ldb, (long)ldb, (long)nc, (long)ncp, (int)K, p.bbits, L, w.rb, (long)(ncp * K), sgb, s);
            GPX_TRY(emu_tile_update({w.a.base, K, nrp * K, sga}, {w.rb, K, ncp * K, sgb}, w.rr, C + r0 * ldc + c0, ldc, nr, nrp, nc, ncp, K, L, EMU_NO_DIAG, 0, s));
        }
        GPX_HIP(hipGetLastError());
    }
    return 0;
}

// ---- the left-looking solve's share (tsolve.hip, trsm_right_lt_slabs): a persistent residue image of the solved slabs -------------------
// Slab p of the solve takes ONE update of depth K = 1024 p against every solved slab before it.  Each solved slab is split once, with the
// scale its row's bound gave at entry, into the image (ld = 1024 (P - 1) columns, equal row tiles: 2 x 8192 rows at N = M = 16384, not
// 8704 + 7680); every later update reads columns 0 .. K of it through the int8 kernel's row stride.  abits / bbits come from the deepest
// K of the call, so one image serves every depth.
bool emu_left_route(bool bounded, bool few, bool ready, int64_t slabs)
{
    static const int on = [] { const char *e = getenv("GPX_EMU_LEFT"); return e ? atoi(e) : 1; }();   // (default 1)
    return bounded && !few && ready && slabs >= 5 && on && emu_enabled(4 * EMU_SLAB);
}

EmuPlan emu_left_plan(int64_t rows, int64_t slabs, int64_t tile_rows)
{
    EmuPlan p = emu_plan_begin(EMU_SLAB * (slabs - 1), false);
    EmuImage &a = p.a;
    a.rows_pad = round_up(rows, EMU_BT);
    int64_t cap = emu_cap(a.ld, (int)a.L);
    if (tile_rows > 0) cap = std::min(cap, round_up(tile_rows, EMU_BT));
    a.tiles = (a.rows_pad + cap - 1) / cap;
    a.rt = round_up((a.rows_pad + a.tiles - 1) / a.tiles, EMU_BT);
    p.ct = EMU_SLAB;
    p.need = {a.tiles * a.rt * a.ld * a.L, p.ct * a.ld * a.L, a.rt * p.ct * a.L, a.rows_pad + EMU_SLAB + 1, a.rows_pad};
    return p;
}

// the row scales of one chunk from its bounds (device, `rows` of them; the padding rows take bound 0), status cleared
int emu_left_begin(const EmuFrame &w, const double *bound, int64_t rows, hipStream_t s)
{
    if (rows > w.a.rows_pad) { gpx_set_error("emu_left_begin: %ld rows in a workspace of %ld", (long)rows, (long)w.a.rows_pad); return GPX_ERR_STATE; }
    GPX_HIP(hipMemsetAsync(w.status(), 0, sizeof(int), s));
    hipLaunchKernelGGL(emu_scale_from_bound_kernel, dim3((unsigned)((w.a.rows_pad + 255) / 256)), dim3(256), 0, s, bound, (long)rows, (long)w.a.rows_pad,
                       w.abits, w.sig, w.status());
    GPX_HIP(hipGetLastError());
    return 0;
}

// solved slab q (X: its first column, `rows` rows, 1024 columns) into the image
int emu_left_split(const EmuFrame &w, const double *X, int64_t ldx, int64_t rows, int64_t q, hipStream_t s)
{
    for (int64_t t = 0, r0 = 0; r0 < rows; ++t, r0 += w.a.rt) {
        const int64_t nr = std::min(w.a.rt, rows - r0), nrp = round_up(nr, EMU_BT);
        emu_launch_split_fixed(X + r0 * ldx, (long)ldx, (long)nr, (long)nrp, EMU_SLAB, w.abits, (int)w.a.L, w.a.tile(t) + q * EMU_SLAB, (long)w.a.ld,
                               (long)w.a.plane(), w.sig + r0, w.status(), s);
    }
    GPX_HIP(hipGetLastError());
    return 0;
}

// C[rows, cols] -= Zs[:, 0:K) B[cols, K]^T with Zs read from the image (K = 1024 p, cols <= 1024): split B (its scales, then its
// residues), then the tile step per row tile
int emu_left_update(const EmuFrame &w, const double *B, int64_t ldb, double *C, int64_t ldc, int64_t rows, int64_t cols, int64_t K, hipStream_t s,
                    Profiler *prof)
{
    if (K <= 0 || K > w.a.ld || K % EMU_SLAB || cols <= 0 || cols > EMU_SLAB || rows > w.a.rows_pad) {
        gpx_set_error("emu_left_update: %ld x %ld x %ld outside the image", (long)rows, (long)cols, (long)K);
        return GPX_ERR_STATE;
    }
    GPX_TRY(emu_fits(w, w, "emu_left_update"));
    ProfScope ps(prof, s, GPX_K_GEMM_EMU, 2.0 * (double)rows * (double)cols * (double)K);
    const int64_t ncp = round_up(cols, EMU_BT);
    const EmuOperand b{w.rb, K, ncp * K, w.sig + w.a.rows_pad};
    emu_launch_split(B, (long)ldb, (long)cols, (long)ncp, (int)K, w.bbits, (int)w.a.L, w.rb, (long)b.plane, w.sig + w.a.rows_pad, s);
    for (int64_t r0 = 0; r0 < rows; r0 += w.a.rt) {
        const int64_t nr = std::min(w.a.rt, rows - r0), nrp = round_up(nr, EMU_BT);
        GPX_TRY(emu_tile_update(w.a.from_row(r0, w.sig), b, w.rr, C + r0 * ldc, ldc, nr, nrp, cols, ncp, K, (int)w.a.L, EMU_NO_DIAG, 0, s));
    }
    GPX_HIP(hipGetLastError());
    return 0;
}

// ---- the symmetric update of the factorisation's far columns (chol.hip, Lookahead::group_boundary) -------------------------------------
// C[i, j] -= sum_k A[i, k] A[j, k] for j <= i < rows, by column panels of 1024.  A is split ONCE, every row with its own maximum and
// the same bit count emu_scale_bits(K, L) / 2 in either role, into the image (ld = K): column panel q's B operand is rows q 1024 .. of
// that image.  rt is a multiple of 1024 wherever there is more than one row tile, so a panel's B rows never straddle two.  Per column
// panel and row tile below it the tile step, whose rebuild ends every row at the diagonal: nothing above it is written.
EmuPlan emu_syrk_plan(int64_t rows, int64_t K, int64_t tile_rows)
{
    EmuPlan p = emu_plan_begin(K, true);
    EmuImage &a = p.a;
    a.rows_pad = round_up(rows, EMU_BT);
    int64_t cap = std::max<int64_t>(EMU_SLAB, emu_cap(K, (int)a.L) / EMU_SLAB * EMU_SLAB);
    if (tile_rows > 0) cap = std::min(cap, round_up(tile_rows, EMU_SLAB));
    a.rt = std::min(a.rows_pad, cap);
    a.tiles = (a.rows_pad + a.rt - 1) / a.rt;
    p.ct = std::min<int64_t>(EMU_SLAB, a.rows_pad);
    p.need = {a.tiles * a.rt * K * a.L, 0, a.rt * p.ct * a.L, a.rows_pad, 0};
    return p;
}

// rows of A (the geometry of the plan in use) into the image, row scales into w.sig
int emu_syrk_split(const EmuFrame &w, const double *A, int64_t lda, int64_t rows, hipStream_t s)
{
    GPX_TRY(emu_fits(w, w, "emu_syrk_split"));
    for (int64_t t = 0, r0 = 0; r0 < w.a.rows_pad; ++t, r0 += w.a.rt) {
        const int64_t nrp = std::min(w.a.rt, w.a.rows_pad - r0), nr = std::max<int64_t>(0, std::min(nrp, rows - r0));
        emu_launch_split(A + r0 * lda, (long)lda, (long)nr, (long)nrp, (int)w.a.ld, w.abits, (int)w.a.L, w.a.tile(t), (long)w.a.plane(), w.sig + r0, s);
    }
    GPX_HIP(hipGetLastError());
    return 0;
}

// column panel q: C[i, j] for q 1024 <= j < min(rows, (q + 1) 1024), j <= i < rows (C: the matrix's first entry)
// diag_tile (1 or a power of two that divides 1024): row i ends at the last column of its diag_tile x diag_tile diagonal block -- the
// factorisation's diagonal tiles stay symmetric in full, as its fp64 updates leave them (the products are symmetric to the bit)
int emu_syrk_panel(const EmuFrame &w, int64_t q, double *C, int64_t ldc, int64_t rows, hipStream_t s, Profiler *prof, int diag_tile)
{
    const EmuImage &a = w.a;
    const int64_t q0 = q * EMU_SLAB, nc = std::min<int64_t>(EMU_SLAB, rows - q0), ncp = round_up(nc, EMU_BT);
    if (nc <= 0) return 0;
    GPX_TRY(emu_fits(w, w, "emu_syrk_panel"));
    ProfScope ps(prof, s, GPX_K_GEMM_EMU, 2.0 * (double)(rows - q0) * (double)nc * (double)a.ld);
    for (int64_t t = q0 / a.rt; t < a.tiles; ++t) {
        const int64_t lo = std::max(t * a.rt, q0), hi = std::min((t + 1) * a.rt, a.rows_pad), nrp = hi - lo, nr = std::min(hi, rows) - lo;
        if (nr <= 0) break;
        GPX_TRY(emu_tile_update(a.from_row(lo, w.sig), a.from_row(q0, w.sig), w.rr, C + lo * ldc + q0, ldc, nr, nrp, nc, ncp, a.ld, (int)a.L, lo - q0,
                                diag_tile - 1, s));
    }
    GPX_HIP(hipGetLastError());
    return 0;
}

// ---- C-ABI: the emulated product on caller device buffers (tests), the int8 product kernel alone on random residues (its rate) -------
// the symmetric update: any K that is a multiple of 128 below 2^17; tile_rows > 0: a smaller row tile (rounded up to 1024), for tests
// diag_tile: emu_syrk_panel's; plan_rows > rows: the workspace is reserved and allocated for plan_rows rows and the plan of `rows` used
// for the split, as the factorisation does for every group boundary after its largest (chol.hip); column panels in ascending order
extern "C" int gpx_emu_syrk_lower_sub_ex(const double *A, int64_t lda, int64_t rows, int64_t K, double *C, int64_t ldc, int64_t tile_rows, int diag_tile,
                                         int64_t plan_rows)
{
    GPX_TRY(gpx_require_device());
    if (rows < 0 || tile_rows < 0 || !A || !C || diag_tile < 1 || (diag_tile & (diag_tile - 1)) || EMU_SLAB % diag_tile || (plan_rows && plan_rows < rows)) {
        gpx_set_error("gpx_emu_syrk_lower_sub: bad arguments");
        return GPX_ERR_BAD_ARG;
    }
    GPX_TRY(emu_check_args(A, lda, A, lda, ldc, rows, K));
    if (rows == 0) return 0;
    EmuFrame w;
    w.reserve(emu_syrk_plan(std::max(rows, plan_rows), K, tile_rows));
    if (emu_alloc(w, nullptr)) return GPX_ERR_HIP;
    w.use(emu_syrk_plan(rows, K, tile_rows));
    int rc = emu_syrk_split(w, A, lda, rows, 0);
    for (int64_t q = 0; !rc && q * EMU_SLAB < rows; ++q) rc = emu_syrk_panel(w, q, C, ldc, rows, 0, nullptr, diag_tile);
    if (hipStreamSynchronize(0) != hipSuccess && rc == 0) { gpx_set_error("gpx_emu_syrk_lower_sub: stream failed"); rc = GPX_ERR_HIP; }
    emu_free(w);
    return rc;
}

extern "C" int gpx_emu_syrk_lower_sub(const double *A, int64_t lda, int64_t rows, int64_t K, double *C, int64_t ldc, int64_t tile_rows)
{
    return gpx_emu_syrk_lower_sub_ex(A, lda, rows, K, C, ldc, tile_rows, 1, 0);
}

extern "C" int gpx_emu_gemm_nt_sub(const double *A, int64_t lda, const double *B, int64_t ldb, double *C, int64_t ldc, int64_t rows, int64_t cols,
                                   int64_t K)
{
    GPX_TRY(gpx_require_device());
    if (rows < 0 || cols < 0 || !A || !B || !C) { gpx_set_error("gpx_emu_gemm_nt_sub: bad arguments"); return GPX_ERR_BAD_ARG; }
    GPX_TRY(emu_check_args(A, lda, B, ldb, ldc, cols, K));   // before the workspace is sized and allocated
    if (rows == 0 || cols == 0) return 0;
    Scratch sc(0);
    EmuFrame w;
    w.reserve(emu_work_plan(rows, cols, K));
    GPX_TRY(emu_alloc(w, &sc));
    int rc = emu_gemm_nt_sub(A, lda, B, ldb, C, ldc, rows, cols, K, w, 0, nullptr);
    if (hipStreamSynchronize(0) != hipSuccess && rc == 0) { gpx_set_error("gpx_emu_gemm_nt_sub: stream failed"); rc = GPX_ERR_HIP; }
    return rc;
}

// The two integer kernels alone on caller device buffers (tests/test_emulated_rebuild.py).  Synchronous.
// diag, dmask: the kernel's -- row i ends at column (i + diag) | dmask (dmask + 1 a power of two), or at cols - 1 if that is smaller
extern "C" int gpx_emu_rebuild_ex(const int8_t *R, int64_t ldr, int64_t sr, int nmod, const int *sa, const int *sb, double *C, int64_t ldc, int64_t rows,
                                  int64_t cols, int64_t diag, int64_t dmask)
{
    GPX_TRY(gpx_require_device());
    // the kernel reads four residue bytes at once, also in the column tail: rows of R are 4-byte aligned and padded to a multiple of 4
    if (!R || !sa || !sb || !C || rows < 0 || cols < 0 || nmod < 2 || nmod > EMU_MAXL || ldr < round_up(cols, 4) || (ldr | sr) & 3 ||
        (uintptr_t)R & 3 || sr < rows * ldr || ldc < cols || dmask < 0 || (dmask & (dmask + 1)) || diag < -EMU_NO_DIAG || diag > EMU_NO_DIAG) {
        gpx_set_error("gpx_emu_rebuild: bad arguments");
        return GPX_ERR_BAD_ARG;
    }
    if (rows == 0 || cols == 0) return 0;
    emu_launch_rebuild(R, ldr, sr, nmod, sa, sb, C, ldc, rows, cols, diag, dmask, 0);
    GPX_HIP(hipGetLastError());
    GPX_HIP(hipStreamSynchronize(0));
    return 0;
}

extern "C" int gpx_emu_rebuild(const int8_t *R, int64_t ldr, int64_t sr, int nmod, const int *sa, const int *sb, double *C, int64_t ldc, int64_t rows,
                               int64_t cols)
{
    return gpx_emu_rebuild_ex(R, ldr, sr, nmod, sa, sb, C, ldc, rows, cols, EMU_NO_DIAG, 0);
}

// The two splits alone on caller device buffers (tests/test_emulated_split.py).  Synchronous.
static bool emu_split_args_ok(const double *X, int64_t ldx, int64_t rows, int64_t rows_pad, int64_t width, int bits, int nmod, const int8_t *res,
                              int64_t ldr, int64_t plane, const int *sig)
{
    return X && res && sig && rows >= 0 && rows <= rows_pad && rows_pad < ((int64_t)1 << 31) && width > 0 && bits >= 1 && bits <= 59 && nmod >= 1 &&
           nmod <= EMU_MAXL && ldx >= width && !(ldx & 1) && !((uintptr_t)X & 15) && !((uintptr_t)res & 15) && ldr >= width && !(ldr & 15) &&
           !(plane & 15) && plane >= (rows_pad - 1) * ldr + width;
}

extern "C" int gpx_emu_split(const double *X, int64_t ldx, int64_t rows, int64_t rows_pad, int64_t K, int bits, int nmod, int8_t *res, int64_t plane,
                             int *sig)
{
    GPX_TRY(gpx_require_device());
    if (!emu_k_ok(K) || !emu_split_args_ok(X, ldx, rows, rows_pad, K, bits, nmod, res, K, plane, sig)) {
        gpx_set_error("gpx_emu_split: bad arguments");
        return GPX_ERR_BAD_ARG;
    }
    if (rows_pad == 0) return 0;
    emu_launch_split(X, (long)ldx, (long)rows, (long)rows_pad, (int)K, bits, nmod, res, (long)plane, sig, 0);
    GPX_HIP(hipGetLastError());
    GPX_HIP(hipStreamSynchronize(0));
    return 0;
}

extern "C" int gpx_emu_split_fixed(const double *X, int64_t ldx, int64_t rows, int64_t rows_pad, int64_t width, int bits, int nmod, int8_t *res,
                                   int64_t ldr, int64_t plane, int *sig, int *status)
{
    GPX_TRY(gpx_require_device());
    if (!status || width % 16 || width > EMU_SLAB || !emu_split_args_ok(X, ldx, rows, rows_pad, width, bits, nmod, res, ldr, plane, sig)) {
        gpx_set_error("gpx_emu_split_fixed: bad arguments");
        return GPX_ERR_BAD_ARG;
    }
    if (rows_pad == 0) return 0;
    emu_launch_split_fixed(X, (long)ldx, (long)rows, (long)rows_pad, (int)width, bits, nmod, res, (long)ldr, (long)plane, sig, status, 0);
    GPX_HIP(hipGetLastError());
    GPX_HIP(hipStreamSynchronize(0));
    return 0;
}

// A: planes of [rows][lda] bytes (lda >= K, a multiple of 16; 256 lda < 2^31: a panel's 32-bit byte offsets), B: dense planes of [cols][K],
// R: planes of [rows][ldr] bytes (ldr >= cols; any R and ldr: byte stores)
extern "C" int gpx_emu_i8_gemm_ld(const int8_t *A, int64_t lda, const int8_t *B, int64_t rows, int64_t cols, int64_t K, int nmod, int8_t *R,
                                  int64_t ldr)
{
    GPX_TRY(gpx_require_device());
    if (!A || !B || !R || rows <= 0 || cols <= 0 || rows % EMU_BT || cols % EMU_BT || !emu_k_ok(K) || nmod < 1 ||
        nmod > EMU_MAXL || ((uintptr_t)A | (uintptr_t)B) & 15 || rows / EMU_BT * (cols / EMU_BT) * nmod > INT32_MAX || lda < K || lda & 15 ||
        (EMU_BT - 1) * lda + K >= ((int64_t)1 << 31) || ldr < cols) {
        gpx_set_error("gpx_emu_i8_gemm: bad arguments");
        return GPX_ERR_BAD_ARG;
    }
    GPX_TRY(emu_launch_product({A, lda, rows * lda, nullptr}, {B, K, cols * K, nullptr}, R, ldr, rows * ldr, rows / EMU_BT, cols / EMU_BT, K, nmod, 0));
    GPX_HIP(hipGetLastError());
    GPX_HIP(hipStreamSynchronize(0));
    return 0;
}

extern "C" int gpx_emu_i8_gemm(const int8_t *A, const int8_t *B, int64_t rows, int64_t cols, int64_t K, int nmod, int8_t *R)
{
    return gpx_emu_i8_gemm_ld(A, K, B, rows, cols, K, nmod, R, cols);
}

__global__ void emu_fill_kernel(int8_t *p, long n, unsigned seed)
{
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long)gridDim.x * 256) {
        unsigned x = (unsigned)i * 2654435761u ^ seed;
        x ^= x >> 15; x *= 2246822519u; x ^= x >> 13;
        p[i] = (int8_t)(x & 0xff);
    }
}

extern "C" int gpx_bench_emu_i8(int64_t rows, int64_t cols, int64_t K, int nmod, int iters, double *ms)
{
    GPX_TRY(gpx_require_device());
    if (rows % EMU_BT || cols % EMU_BT || !emu_k_ok(K) || nmod < 1 || nmod > EMU_MAXL || iters < 1 || !ms) {
        gpx_set_error("gpx_bench_emu_i8: bad arguments");
        return GPX_ERR_BAD_ARG;
    }
    Scratch sc(0);
    int8_t *wa = nullptr, *wb = nullptr, *wr = nullptr;
    int rc = 0;
    GPX_TRY(sc.take(&wa, rows * K * nmod));
    GPX_TRY(sc.take(&wb, cols * K * nmod));
    GPX_TRY(sc.take(&wr, rows * cols * nmod));
    hipLaunchKernelGGL(emu_fill_kernel, dim3(4096), dim3(256), 0, 0, wa, (long)(rows * K * nmod), 1u);
    hipLaunchKernelGGL(emu_fill_kernel, dim3(4096), dim3(256), 0, 0, wb, (long)(cols * K * nmod), 2u);
    hipEvent_t e0 = nullptr, e1 = nullptr;
    float t = 0.0f;
    hipError_t e = hipEventCreate(&e0);
    if (e == hipSuccess) e = hipEventCreate(&e1);
    for (int it = -1; it < iters && e == hipSuccess; ++it) {   // it = -1: warm-up
        if (it == 0) e = hipEventRecord(e0, 0);
        rc = emu_launch_product({wa, K, rows * K, nullptr}, {wb, K, cols * K, nullptr}, wr, cols, rows * cols, rows / EMU_BT, cols / EMU_BT, K, nmod, 0);
        if (rc) break;
        if (e == hipSuccess) e = hipGetLastError();
    }
    if (e == hipSuccess) e = hipEventRecord(e1, 0);
    if (e == hipSuccess) e = hipEventSynchronize(e1);
    if (e == hipSuccess) e = hipEventElapsedTime(&t, e0, e1);
    if (e != hipSuccess) { gpx_set_error("gpx_bench_emu_i8: %s", hipGetErrorString(e)); rc = GPX_ERR_HIP; }
    *ms = t / iters;
    if (e0) (void)hipEventDestroy(e0);
    if (e1) (void)hipEventDestroy(e1);
    (void)hipDeviceSynchronize();
    return rc;
}
