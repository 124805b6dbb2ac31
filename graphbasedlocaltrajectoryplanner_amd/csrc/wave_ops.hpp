// wave_ops.hpp -- cross-lane primitives of a wave64 on gfx950 (DPP row operations, v_permlane16_swap / v_permlane32_swap): minima, maxima,
// arg-minima and the exclusive scan that the path kernel and the velocity stage share, their self-check kernel (k_exp_wave_ops), the
// wave-scope LDS hand-over and normalize_psi_dev. Included by ltpl_hip.hip in front of paths_team.hpp; no include guard games: one
// translation unit.
#pragma once
// ---------------------------------------------------------------------------------------------------------------------
// wave helpers (wave64)
// ---------------------------------------------------------------------------------------------------------------------
// CROSS-LANE MOVES ON THE VECTOR ALU (round 5). `__shfl_xor` / `__shfl_up` compile to ds_bpermute_b32: an LDS-pipe instruction with an LDS
// round trip of latency per step, in kernels whose LDS pipe is a co-limiter and whose waves spend ~46 % of their cycles in s_waitcnt
// (275 of the 907 static LDS-pipe instructions of the round-4 batch path kernel were ds_bpermute). The reductions and scans below exchange
// through DPP row operations (partner at distance 1, 2, 4, 8 inside a row of 16 lanes) and the gfx950 row / half swaps
// (v_permlane16_swap, v_permlane32_swap: distance 16 and 32) instead: no LDS instruction, no lgkmcnt wait.
// ALL 64 LANES MUST BE ACTIVE at the call (wave-uniform control flow): a DPP move from an inactive lane delivers no data.
// (the round-4 `__shfl_xor` forms: tools/experiments/r05_lost_switches.patch)
#if defined(__HIP_DEVICE_COMPILE__) && !defined(__gfx950__)
#error "the DPP / v_permlane16_swap / v_permlane32_swap reductions below are gfx950 code: build with --offload-arch=gfx950 (the round-4 shuffle forms: tools/experiments/r05_lost_switches.patch)"
#endif
#define DPP_XOR1 0xB1                   // quad_perm:[1,0,3,2]
#define DPP_XOR2 0x4E                   // quad_perm:[2,3,0,1]
#define DPP_HALF_MIRROR 0x141           // lane i <-> 7 - i  of every 8: the partner at distance 4 once the quads are uniform
#define DPP_MIRROR 0x140                // lane i <-> 15 - i of every 16: the partner at distance 8 once the halves of 8 are uniform
#define DPP_ROR8 0x128                  // row_ror:8 = lane i ^ 8
#define DPP_SHL4 0x104                  // row_shl:4 (lane i <- lane i + 4)
#define DPP_SHR(n) (0x110 + (n))        // row_shr:n (lane i <- lane i - n inside the row)
#define DPP_BCAST15 0x142               // lane 15 of every row -> the next row
#define DPP_BCAST31 0x143               // lane 31 -> rows 2 and 3
typedef unsigned lane_pair_t __attribute__((ext_vector_type(2)));
template <int CTRL> __device__ __forceinline__ int dpp_i32(int v) { return __builtin_amdgcn_mov_dpp(v, CTRL, 0xf, 0xf, false); }
template <int CTRL> __device__ __forceinline__ double dpp_f64(double v)
{
    return __hiloint2double(dpp_i32<CTRL>(__double2hiint(v)), dpp_i32<CTRL>(__double2loint(v)));
}
// the value of lane (i ^ M), M = 1, 2, 4, 8, for ANY lane contents (the mirror forms above need uniform sub-groups)
template <int M> __device__ __forceinline__ int xor_i32(int v)
{
    if constexpr (M == 1) return dpp_i32<DPP_XOR1>(v);
    else if constexpr (M == 2) return dpp_i32<DPP_XOR2>(v);
    else if constexpr (M == 4) {           // banks (= quads of a row) 0, 2 take the quad above, banks 1, 3 the quad below
        const int up = __builtin_amdgcn_update_dpp(v, v, DPP_SHL4, 0xf, 0x5, false);
        return __builtin_amdgcn_update_dpp(up, v, DPP_SHR(4), 0xf, 0xa, false);
    } else { static_assert(M == 8, "distance inside a row"); return dpp_i32<DPP_ROR8>(v); }
}
template <int M> __device__ __forceinline__ double xor_f64(double v) { return __hiloint2double(xor_i32<M>(__double2hiint(v)), xor_i32<M>(__double2loint(v))); }
// distance 16 / 32: with both operands = v the swap returns, in every lane i, the pair {v[i], v[i ^ M]} (in an order that depends on the
// lane's half) -- symmetric combinations (min, lexicographic min) need not know which is which
template <int M> __device__ __forceinline__ lane_pair_t swap_pair(unsigned v)
{
    if constexpr (M == 16) return __builtin_amdgcn_permlane16_swap(v, v, false, false);
    else { static_assert(M == 32, "row / half swap"); return __builtin_amdgcn_permlane32_swap(v, v, false, false); }
}
template <int M> __device__ __forceinline__ void swap_pair_f64(double v, double& a, double& b)
{
    const lane_pair_t lo = swap_pair<M>((unsigned)__double2loint(v)), hi = swap_pair<M>((unsigned)__double2hiint(v));
    a = __hiloint2double((int)hi.x, (int)lo.x); b = __hiloint2double((int)hi.y, (int)lo.y);
}

// minimum of a double over the wave (no NaN among the keys), in every lane. The first key decides nearly always, so the callers reduce it
// alone and fall back to wave_min3 only when it is attained more than once.
__device__ __forceinline__ double wave_min_f64(double k)
{
    k = __builtin_fmin(k, dpp_f64<DPP_XOR1>(k));
    k = __builtin_fmin(k, dpp_f64<DPP_XOR2>(k));
    k = __builtin_fmin(k, dpp_f64<DPP_HALF_MIRROR>(k));
    k = __builtin_fmin(k, dpp_f64<DPP_MIRROR>(k));
    double a, b;
    swap_pair_f64<16>(k, a, b); k = __builtin_fmin(a, b);
    swap_pair_f64<32>(k, a, b); k = __builtin_fmin(a, b);
    return k;
}
__device__ __forceinline__ int wave_min_i32(int k)
{
    k = min(k, dpp_i32<DPP_XOR1>(k));
    k = min(k, dpp_i32<DPP_XOR2>(k));
    k = min(k, dpp_i32<DPP_HALF_MIRROR>(k));
    k = min(k, dpp_i32<DPP_MIRROR>(k));
    lane_pair_t r = swap_pair<16>((unsigned)k); k = min((int)r.x, (int)r.y);
    r = swap_pair<32>((unsigned)k); k = min((int)r.x, (int)r.y);
    return k;
}
__device__ __forceinline__ int wave_max_i32(int k)
{
    k = max(k, dpp_i32<DPP_XOR1>(k));
    k = max(k, dpp_i32<DPP_XOR2>(k));
    k = max(k, dpp_i32<DPP_HALF_MIRROR>(k));
    k = max(k, dpp_i32<DPP_MIRROR>(k));
    lane_pair_t r = swap_pair<16>((unsigned)k); k = max((int)r.x, (int)r.y);
    r = swap_pair<32>((unsigned)k); k = max((int)r.x, (int)r.y);
    return k;
}
// maximum over every group of eight lanes (lanes 8 k .. 8 k + 7), in each of its lanes
__device__ __forceinline__ int oct_max_i32(int k)
{
    k = max(k, dpp_i32<DPP_XOR1>(k));
    k = max(k, dpp_i32<DPP_XOR2>(k));
    return max(k, dpp_i32<DPP_HALF_MIRROR>(k));
}
// lexicographic minimum over (k1, k2, idx) / (k, idx): one exchange step at distance M (true partner: the keys differ from lane to lane)
template <int M> __device__ __forceinline__ void min3_step(double& k1, double& k2, int& idx)
{
    if constexpr (M < 16) {
        const double o1 = xor_f64<M>(k1), o2 = xor_f64<M>(k2); const int oi = xor_i32<M>(idx);
        const bool take = (o1 < k1) || (o1 == k1 && ((o2 < k2) || (o2 == k2 && oi < idx)));
        if (take) { k1 = o1; k2 = o2; idx = oi; }
    } else {
        double a1, b1, a2, b2; swap_pair_f64<M>(k1, a1, b1); swap_pair_f64<M>(k2, a2, b2);
        const lane_pair_t ri = swap_pair<M>((unsigned)idx);
        const int ai = (int)ri.x, bi = (int)ri.y;
        const bool take_b = (b1 < a1) || (b1 == a1 && ((b2 < a2) || (b2 == a2 && bi < ai)));
        k1 = take_b ? b1 : a1; k2 = take_b ? b2 : a2; idx = take_b ? bi : ai;
    }
}
template <int M> __device__ __forceinline__ void min2_step(double& k, int& idx)
{
    if constexpr (M < 16) {
        const double o = xor_f64<M>(k); const int oi = xor_i32<M>(idx);
        const bool take = (o < k) || (o == k && oi < idx);
        if (take) { k = o; idx = oi; }
    } else {
        double a, b; swap_pair_f64<M>(k, a, b);
        const lane_pair_t ri = swap_pair<M>((unsigned)idx);
        const int ai = (int)ri.x, bi = (int)ri.y;
        const bool take_b = (b < a) || (b == a && bi < ai);
        k = take_b ? b : a; idx = take_b ? bi : ai;
    }
}
__device__ __forceinline__ void wave_min3(double& k1, double& k2, int& idx)
{
    min3_step<1>(k1, k2, idx); min3_step<2>(k1, k2, idx); min3_step<4>(k1, k2, idx); min3_step<8>(k1, k2, idx);
    min3_step<16>(k1, k2, idx); min3_step<32>(k1, k2, idx);
}
// the same for (key, index) pairs: the closest-point searches carry no second key
__device__ __forceinline__ void wave_min2(double& k, int& idx)
{
    min2_step<1>(k, idx); min2_step<2>(k, idx); min2_step<4>(k, idx); min2_step<8>(k, idx); min2_step<16>(k, idx); min2_step<32>(k, idx);
}
// ... over the lanes that agree in their low bits (lane & (np2 - 1)): the steps at distance >= np2 only (np2 a power of two, uniform)
__device__ __forceinline__ void wave_min2_from(double& k, int& idx, int np2)
{
    if (np2 <= 1) min2_step<1>(k, idx);
    if (np2 <= 2) min2_step<2>(k, idx);
    if (np2 <= 4) min2_step<4>(k, idx);
    if (np2 <= 8) min2_step<8>(k, idx);
    if (np2 <= 16) min2_step<16>(k, idx);
    if (np2 <= 32) min2_step<32>(k, idx);
}

// exclusive prefix sum of an int over the wave (+ the total): Hillis-Steele inside the rows (row_shr, lanes without a source add 0), then
// the row totals through the two broadcast forms
__device__ __forceinline__ int wave_excl_scan(int v, int lane, int& total)
{
    (void)lane;
    int x = v;
    x += __builtin_amdgcn_update_dpp(0, x, DPP_SHR(1), 0xf, 0xf, true);
    x += __builtin_amdgcn_update_dpp(0, x, DPP_SHR(2), 0xf, 0xf, true);
    x += __builtin_amdgcn_update_dpp(0, x, DPP_SHR(4), 0xf, 0xf, true);
    x += __builtin_amdgcn_update_dpp(0, x, DPP_SHR(8), 0xf, 0xf, true);
    x += __builtin_amdgcn_update_dpp(0, x, DPP_BCAST15, 0xa, 0xf, false);      // rows 1 and 3 += total of the row below
    x += __builtin_amdgcn_update_dpp(0, x, DPP_BCAST31, 0xc, 0xf, false);      // rows 2 and 3 += total of rows 0 and 1
    total = __builtin_amdgcn_readlane(x, 63);
    return x - v;
}

// Self-check of the cross-lane helpers above: every helper against a plain loop over the wave's values in LDS. err[0] = number of lanes that
// disagree. Part of the create-time self-test of the product library since round 6 (wave_ops_selftest: the helpers are DPP / permlane-swap code
// that only exists for gfx950 and assumes 64 active lanes); tests/test_gpu_wave_ops.py drives it with its own data through the experiment build.
__global__ __launch_bounds__(64) void k_exp_wave_ops(const double* vals, const int* ivals, int rounds, int* err)
{
    __shared__ double sd[64], sd2[64];
    __shared__ int si[64];
    const int lane = threadIdx.x;
    int bad = 0;
    for (int r = 0; r < rounds; ++r) {
        const double d = vals[(size_t)r * 128 + lane], d2 = vals[(size_t)r * 128 + 64 + lane];
        const int iv = ivals[(size_t)r * 64 + lane];
        sd[lane] = d; sd2[lane] = d2; si[lane] = iv;
        __syncthreads();
        double rmin = INFINITY; int imin = 0x7fffffff, imax = -0x7fffffff - 1, isum = 0, ipre = 0, omax = -0x7fffffff - 1;
        double a1 = INFINITY, a2 = INFINITY; int ai = 0x7fffffff;          // lexicographic minimum over (d, d2, iv)
        double b1 = INFINITY; int bi = 0x7fffffff;                          // ... over (d, iv)
        for (int l = 0; l < 64; ++l) {
            rmin = sd[l] < rmin ? sd[l] : rmin; imin = si[l] < imin ? si[l] : imin; imax = si[l] > imax ? si[l] : imax;
            isum += si[l] & 0xff; if (l < lane) ipre += si[l] & 0xff;
            if ((l >> 3) == (lane >> 3)) omax = si[l] > omax ? si[l] : omax;
            if (sd[l] < a1 || (sd[l] == a1 && (sd2[l] < a2 || (sd2[l] == a2 && si[l] < ai)))) { a1 = sd[l]; a2 = sd2[l]; ai = si[l]; }
            if (sd[l] < b1 || (sd[l] == b1 && si[l] < bi)) { b1 = sd[l]; bi = si[l]; }
        }
        if (wave_min_f64(d) != rmin) ++bad;
        if (wave_min_i32(iv) != imin) ++bad;
        if (wave_max_i32(iv) != imax) ++bad;
        if (oct_max_i32(iv) != omax) ++bad;
        { int tot; const int ex = wave_excl_scan(iv & 0xff, lane, tot); if (ex != ipre || tot != isum) ++bad; }
        { double k1 = d, k2 = d2; int ix = iv; wave_min3(k1, k2, ix); if (k1 != a1 || k2 != a2 || ix != ai) ++bad; }
        { double k = d; int ix = iv; wave_min2(k, ix); if (k != b1 || ix != bi) ++bad; }
        for (int np2 = 1; np2 <= 64; np2 <<= 1) {                            // segment merge of phase 1: lanes with equal (lane & (np2 - 1))
            double k = d; int ix = iv; wave_min2_from(k, ix, np2);
            double c1 = INFINITY; int ci = 0x7fffffff;
            for (int l = lane & (np2 - 1); l < 64; l += np2) if (sd[l] < c1 || (sd[l] == c1 && si[l] < ci)) { c1 = sd[l]; ci = si[l]; }
            if (k != c1 || ix != ci) ++bad;
        }
        __syncthreads();
    }
    if (bad) atomicAdd(err, 1);
}

// LDS hand-over between the lanes of ONE wave: DS operations of a wave execute in order, so only the compiler has to be
// kept from reordering (wavefront-scope fences emit no s_waitcnt vmcnt and do not serialise outstanding global loads)
__device__ __forceinline__ void wave_sync_lds()
{
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

__device__ __forceinline__ double normalize_psi_dev(double psi)
{
    double sgn = (psi > 0.0) ? 1.0 : ((psi < 0.0) ? -1.0 : 0.0);
    double out = sgn * fmod(fabs(psi), 2.0 * D_PI);
    if (out >= D_PI) out -= 2.0 * D_PI;
    else if (out < -D_PI) out += 2.0 * D_PI;
    return out;
}
