// Paikin-Tal compatibility stage of the reference's puzzle solver (paikin_tal_solver/inter_piece_distance.py): type-1 puzzles first,
// then the kernels of type 2 (pieces of unknown rotation) over (piece, side) candidates.
//
// State, all on the device and owned by the caller (n pieces, side s: top 0, right 1, bottom 2, left 3; s^ = (s + 2) % 4):
//   Dq       int32 [4, n, n]  distance of side s of piece i to side s^ of piece j (the diagonal is never read)
//   min_d, second_d int64 [n, 4]  per (piece, side): the smallest and second-smallest distance, with multiplicity
//   compat   float32 [4, n, n]  asymmetric compatibility C, mutual float32 [4, n, n] mutual compatibility M
//
// Every value is exact and independent of the work split: the min / second-best reductions are integer, C and M are elementwise
// (C in fp64 rounded once to fp32, M = (C + C^) / 2 in fp32, as numpy does it), the start ordering is a rank count, and the slot
// scan is an integer max over packed (order-preserving key, reversed linear index) words.
#include "common.h"
#include "puzzle_turn.h"

#pragma clang fp contract(off)

namespace {

constexpr int THREADS = 256;
constexpr int ROWS_PER_BLOCK = THREADS / VITED_WAVE;
constexpr int64_t PY_MAXSIZE = INT64_MAX;                  // sys.maxsize: the reference's initial second-best distance
constexpr int MAX_PIECES = 46340;                          // n * n fits in int32 (slot-scan indices)

__device__ __forceinline__ int comp_side(int s) { return (s + 2) & 3; }

__device__ __forceinline__ void keep_two_smallest(int64_t& m1, int64_t& m2, int64_t d) {
    if (d < m1) {
        m2 = m1;
        m1 = d;
    } else if (d < m2) {
        m2 = d;
    }
}

// Per (piece i, side s), one wave: the two smallest distances over j != i (RECALC: over unplaced j only), with multiplicity,
// seeded with the reference's (maxsize - 1, maxsize).  Init also stores the best-buddy candidate: the j holding the minimum when
// exactly one j does (the reference keeps every tied j and then treats a side with several as having none).  Recalc skips placed
// rows and flags a piece whose 8 values changed.
template <bool RECALC>
__global__ void __launch_bounds__(THREADS) min_second_kernel(const int* __restrict__ dq, int n, const int* __restrict__ placed,
                                                             int64_t* __restrict__ min_d, int64_t* __restrict__ second_d,
                                                             int* __restrict__ candidate, int* __restrict__ changed) {
    const int row = blockIdx.x * ROWS_PER_BLOCK + threadIdx.x / VITED_WAVE;
    const int lane = threadIdx.x % VITED_WAVE;
    if (row >= 4 * n) return;
    const int s = row / n, i = row % n;
    if (RECALC && placed[i]) return;
    const int* d_row = dq + ((int64_t)s * n + i) * n;
    int64_t m1 = PY_MAXSIZE, m2 = PY_MAXSIZE;
    for (int j = lane; j < n; j += VITED_WAVE) {
        if (j == i || (RECALC && placed[j])) continue;
        keep_two_smallest(m1, m2, d_row[j]);
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        const int64_t b1 = __shfl_xor(m1, off, 64), b2 = __shfl_xor(m2, off, 64);
        const int64_t lo = m1 < b1 ? m1 : b1, hi = m1 < b1 ? b1 : m1;
        m1 = lo;
        m2 = hi < (m2 < b2 ? m2 : b2) ? hi : (m2 < b2 ? m2 : b2);
    }
    // the reference's seeds join once (lanes started from maxsize, which only ever adds copies of the larger seed)
    {
        const int64_t s1 = PY_MAXSIZE - 1, s2 = PY_MAXSIZE;
        const int64_t lo = m1 < s1 ? m1 : s1, hi = m1 < s1 ? s1 : m1;
        const int64_t m2b = m2 < s2 ? m2 : s2;
        m1 = lo;
        m2 = hi < m2b ? hi : m2b;
    }
    const int64_t at = (int64_t)i * 4 + s;
    if (!RECALC) {
        int count = 0, first = n;
        for (int j = lane; j < n; j += VITED_WAVE) {
            if (j != i && d_row[j] == m1) {
                ++count;
                first = first < j ? first : j;
            }
        }
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) {
            count += __shfl_xor(count, off, 64);
            const int f = __shfl_xor(first, off, 64);
            first = first < f ? first : f;
        }
        if (lane == 0) candidate[at] = count == 1 ? first : -1;
    }
    if (lane == 0) {
        if (RECALC && (min_d[at] != m1 || second_d[at] != m2)) changed[i] = 1;
        min_d[at] = m1;
        second_d[at] = m2;
    }
}

// C[s, i, j] (inter_piece_distance.py:359-369): 1 where d == 0, -maxsize where second == 0, else 1 - d / second in fp64.
// Init: every row, diagonal inf.  Recalc: changed rows only, unplaced j only (entries at placed j keep their values).
template <bool RECALC>
__global__ void __launch_bounds__(THREADS) compat_kernel(const int* __restrict__ dq, int n, const int* __restrict__ placed,
                                                         const int* __restrict__ changed, const int64_t* __restrict__ second_d,
                                                         float* __restrict__ compat) {
    const int j = blockIdx.x * THREADS + threadIdx.x;
    const int row = blockIdx.y, s = row / n, i = row % n;
    if (j >= n) return;
    if (RECALC && (!changed[i] || placed[j])) return;
    const int64_t at = ((int64_t)s * n + i) * n + j;
    if (j == i) {
        if (!RECALC) compat[at] = __builtin_inff();
        return;
    }
    const int64_t d = dq[at], sec = second_d[(int64_t)i * 4 + s];
    float c;
    if (d == 0) c = 1.0f;
    else if (sec == 0) c = (float)(-PY_MAXSIZE);
    else c = (float)(1.0 - (double)d / (double)sec);
    compat[at] = c;
}

// M[s, i, j] = M[s^, j, i] = (C[s, i, j] + C[s^, j, i]) / 2 in fp32; the diagonal is inf.  Recalc: pairs with a changed piece.
template <bool RECALC>
__global__ void __launch_bounds__(THREADS) mutual_kernel(const float* __restrict__ compat, int n, const int* __restrict__ changed,
                                                         float* __restrict__ mutual) {
    const int j = blockIdx.x * THREADS + threadIdx.x;
    const int row = blockIdx.y, s = row / n, i = row % n;
    if (j >= n) return;
    if (RECALC && !changed[i] && !changed[j]) return;
    const int64_t at = ((int64_t)s * n + i) * n + j;
    mutual[at] = j == i ? __builtin_inff() : (compat[at] + compat[((int64_t)comp_side(s) * n + j) * n + i]) / 2.0f;
}

// Best buddies (:623-648): the unique candidates that name each other.
__global__ void __launch_bounds__(THREADS) best_buddy_kernel(const int* __restrict__ candidate, int n, int* __restrict__ best_buddy) {
    const int t = blockIdx.x * THREADS + threadIdx.x;
    if (t >= 4 * n) return;
    const int i = t / 4, s = t % 4, j = candidate[t];
    best_buddy[t] = (j >= 0 && candidate[j * 4 + comp_side(s)] == i) ? j : -1;
}

// Start-piece keys (:650-731): count = 4 x (sides with a best buddy) + the best buddies' own counts of such sides, total = the
// mutual compatibilities with those best buddies accumulated in fp32 in side order from 0.
__global__ void __launch_bounds__(THREADS) start_keys_kernel(const int* __restrict__ best_buddy, const float* __restrict__ mutual, int n,
                                                             int* __restrict__ start_count, float* __restrict__ start_total) {
    const int i = blockIdx.x * THREADS + threadIdx.x;
    if (i >= n) return;
    int count = 0;
    float total = 0.0f;
    for (int s = 0; s < 4; ++s) {
        const int j = best_buddy[i * 4 + s];
        if (j < 0) continue;
        count += 4;
        for (int t = 0; t < 4; ++t) count += best_buddy[j * 4 + t] >= 0;
        total = total + mutual[((int64_t)s * n + i) * n + j];
    }
    start_count[i] = count;
    start_total[i] = total;
}

// The stable descending sort of (count, total) as a rank count: piece i goes after every larger key and every equal key of a
// smaller piece id.
__global__ void __launch_bounds__(THREADS) start_order_kernel(const int* __restrict__ start_count, const float* __restrict__ start_total,
                                                              int n, int* __restrict__ start_order) {
    const int i = blockIdx.x * THREADS + threadIdx.x;
    if (i >= n) return;
    const int ci = start_count[i];
    const float ti = start_total[i];
    int rank = 0;
    for (int k = 0; k < n; ++k) {
        const int ck = start_count[k];
        const float tk = start_total[k];
        rank += (ck > ci || (ck == ci && tk > ti) || (ck == ci && tk == ti && k < i));
    }
    start_order[rank] = i;
}

__device__ __forceinline__ uint32_t order_key(float v) {
    if (v == 0.0f) v = 0.0f;                                // -0 and +0 compare equal in the reference
    const uint32_t u = __float_as_uint(v);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}

// Slot scan of _get_next_piece_from_pool (solver.py:456-499): the first maximum of M[s^, p, q] over unplaced pieces p ascending x
// open slots (q, s) in list order.  Each candidate is packed (key(M) << 32) | ~index, so the largest word is the largest value at
// the smallest index; one wave max and one 64-bit atomicMax per wave.
__global__ void __launch_bounds__(THREADS) best_slot_kernel(const float* __restrict__ mutual, int n, const int* __restrict__ placed,
                                                            const int* __restrict__ slot_piece, const int* __restrict__ slot_side, int slots,
                                                            unsigned long long* __restrict__ best) {
    const int64_t total = (int64_t)n * slots;
    unsigned long long word = 0;
    for (int64_t lin = (int64_t)blockIdx.x * THREADS + threadIdx.x; lin < total; lin += (int64_t)gridDim.x * THREADS) {
        const int p = (int)(lin / slots), k = (int)(lin % slots);
        const int q = slot_piece[k];
        if (placed[p] || q < 0 || q >= n) continue;
        const float v = mutual[((int64_t)comp_side(slot_side[k] & 3) * n + p) * n + q];
        const unsigned long long w = ((unsigned long long)order_key(v) << 32) | (0xffffffffu - (uint32_t)lin);
        word = w > word ? w : word;
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        const unsigned long long o = __shfl_xor(word, off, 64);
        word = o > word ? o : word;
    }
    if (threadIdx.x % VITED_WAVE == 0 && word != 0) atomicMax(best, word);
}

// uint32(trunc(fp32(fp32(1 - sigmoid(logit)) * 1000))): the one statement of the quantisation, for both puzzle types.
__device__ __forceinline__ int quantise_logit(float x) {
    const float sig = 1.0f / (1.0f + expf(-x));
    const float q = (1.0f - sig) * 1000.0f;
    return (int)(uint32_t)q;
}

// Ordered-pair distances from the model's 4 logits (evaluation.py:118-133): side s of i uses bin (s + 3) % 4, and the value is
// uint32(trunc(fp32(fp32(1 - sigmoid(logit)) * 1000))).
__global__ void __launch_bounds__(THREADS) distances_kernel(const float* __restrict__ logits, const int64_t* __restrict__ pi,
                                                            const int64_t* __restrict__ pj, int64_t m, int n, int* __restrict__ dq,
                                                            int* __restrict__ bad) {
    const int64_t r = (int64_t)blockIdx.x * THREADS + threadIdx.x;
    if (r >= m) return;
    const int64_t i = pi[r], j = pj[r];
    if (i < 0 || i >= n || j < 0 || j >= n || i == j) {
        atomicOr(bad, 1);
        return;
    }
#pragma unroll
    for (int s = 0; s < 4; ++s) dq[((int64_t)s * n + i) * n + j] = quantise_logit(logits[r * 4 + ((s + 3) & 3)]);
}

// The same quantisation for the learned type-2 path: pair r is (piece i, piece j turned by k clockwise quarter
// turns), jt = k n + j, and its bin b belongs to side (b + 1) % 4 of i against side ((b + 1) % 4 + 2 - k) % 4 of the upright j
// (puzzle_turn.h).  Four turns x four bins fill the 16 pairings of (i, j) once each; k = 0 stores what distances_kernel stores.
__global__ void __launch_bounds__(THREADS) distances2_kernel(const float* __restrict__ logits, const int64_t* __restrict__ pi,
                                                             const int64_t* __restrict__ pjt, int64_t m, int n, int* __restrict__ dq2,
                                                             int* __restrict__ bad) {
    const int64_t r = (int64_t)blockIdx.x * THREADS + threadIdx.x;
    if (r >= m) return;
    const int64_t i = pi[r], jt = pjt[r];
    if (!puzzle_turn::pair_in_range(i, jt, n)) {
        atomicOr(bad, 1);
        return;
    }
#pragma unroll
    for (int b = 0; b < 4; ++b) dq2[puzzle_turn::dq2_slot(n, i, jt, b)] = quantise_logit(logits[r * 4 + b]);
}

// ---- type 2 (inter_piece_distance.py with PuzzleType.type2): any side sj of piece j may meet side si of piece i ---------------------------
// Dq2, compat and mutual are [4, n, n, 4], indexed [si, i, j, sj]: the row of (si, i) holds its 4 n candidates (j, sj) contiguously,
// candidate c = 4 j + sj.  candidate and best_buddy are int32 [n, 4, 2]: (j, sj), or (-1, -1).

// Per (piece i, side si), one wave, each lane one j (its four sj as one 16-byte load): the two smallest distances over the candidates
// with j != i (RECALC: unplaced j only), with multiplicity, seeded as in type 1.  Init also stores how many candidates hold the minimum
// and the candidate itself when exactly one does.
template <bool RECALC>
__global__ void __launch_bounds__(THREADS) min_second2_kernel(const int* __restrict__ dq2, int n, const int* __restrict__ placed,
                                                              int64_t* __restrict__ min_d, int64_t* __restrict__ second_d,
                                                              int* __restrict__ min_count, int* __restrict__ candidate,
                                                              int* __restrict__ changed) {
    const int row = blockIdx.x * ROWS_PER_BLOCK + threadIdx.x / VITED_WAVE;
    const int lane = threadIdx.x % VITED_WAVE;
    if (row >= 4 * n) return;
    const int s = row / n, i = row % n;
    if (RECALC && placed[i]) return;
    const int4* d_row = reinterpret_cast<const int4*>(dq2 + ((int64_t)s * n + i) * n * 4);
    int64_t m1 = PY_MAXSIZE, m2 = PY_MAXSIZE;
    for (int j = lane; j < n; j += VITED_WAVE) {
        if (j == i || (RECALC && placed[j])) continue;
        const int4 d = d_row[j];
        const int v[4] = {d.x, d.y, d.z, d.w};
#pragma unroll
        for (int sj = 0; sj < 4; ++sj) {                    // keep_two_smallest as selects: the lanes stay in registers
            const int64_t x = v[sj];
            m2 = x < m1 ? m1 : (x < m2 ? x : m2);
            m1 = x < m1 ? x : m1;
        }
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        const int64_t b1 = __shfl_xor(m1, off, 64), b2 = __shfl_xor(m2, off, 64);
        const int64_t lo = m1 < b1 ? m1 : b1, hi = m1 < b1 ? b1 : m1;
        m1 = lo;
        m2 = hi < (m2 < b2 ? m2 : b2) ? hi : (m2 < b2 ? m2 : b2);
    }
    {
        const int64_t s1 = PY_MAXSIZE - 1, s2 = PY_MAXSIZE;
        const int64_t lo = m1 < s1 ? m1 : s1, hi = m1 < s1 ? s1 : m1;
        const int64_t m2b = m2 < s2 ? m2 : s2;
        m1 = lo;
        m2 = hi < m2b ? hi : m2b;
    }
    const int64_t at = (int64_t)i * 4 + s;
    if (!RECALC) {
        int count = 0, first = 4 * n;
        for (int j = lane; j < n; j += VITED_WAVE) {
            if (j == i) continue;
            const int4 d = d_row[j];
            const int v[4] = {d.x, d.y, d.z, d.w};
#pragma unroll
            for (int sj = 3; sj >= 0; --sj) {
                if (v[sj] == m1) {
                    ++count;
                    first = first < 4 * j + sj ? first : 4 * j + sj;
                }
            }
        }
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) {
            count += __shfl_xor(count, off, 64);
            const int f = __shfl_xor(first, off, 64);
            first = first < f ? first : f;
        }
        if (lane == 0) {
            min_count[at] = count;
            candidate[at * 2] = count == 1 ? first / 4 : -1;
            candidate[at * 2 + 1] = count == 1 ? first % 4 : -1;
        }
    }
    if (lane == 0) {
        if (RECALC && (min_d[at] != m1 || second_d[at] != m2)) changed[i] = 1;
        min_d[at] = m1;
        second_d[at] = m2;
    }
}

// C[si, i, j, sj], the type-1 expression on the candidate's distance.  One thread per candidate of the row blockIdx.x (4 n rows: the
// dimension that may pass 65535).
template <bool RECALC>
__global__ void __launch_bounds__(THREADS) compat2_kernel(const int* __restrict__ dq2, int n, const int* __restrict__ placed,
                                                          const int* __restrict__ changed, const int64_t* __restrict__ second_d,
                                                          float* __restrict__ compat) {
    const int c = blockIdx.y * THREADS + threadIdx.x;
    const int row = blockIdx.x, s = row / n, i = row % n;
    if (c >= 4 * n) return;
    const int j = c >> 2;
    if (RECALC && (!changed[i] || placed[j])) return;
    const int64_t at = ((int64_t)s * n + i) * n * 4 + c;
    if (j == i) {
        if (!RECALC) compat[at] = __builtin_inff();
        return;
    }
    const int64_t d = dq2[at], sec = second_d[(int64_t)i * 4 + s];
    float v;
    if (d == 0) v = 1.0f;
    else if (sec == 0) v = (float)(-PY_MAXSIZE);
    else v = (float)(1.0 - (double)d / (double)sec);
    compat[at] = v;
}

// M[si, i, j, sj] = M[sj, j, i, si] = (C[si, i, j, sj] + C[sj, j, i, si]) / 2 in fp32; inf at j == i.  Recalc: pairs with a changed piece.
template <bool RECALC>
__global__ void __launch_bounds__(THREADS) mutual2_kernel(const float* __restrict__ compat, int n, const int* __restrict__ changed,
                                                          float* __restrict__ mutual) {
    const int c = blockIdx.y * THREADS + threadIdx.x;
    const int row = blockIdx.x, s = row / n, i = row % n;
    if (c >= 4 * n) return;
    const int j = c >> 2, sj = c & 3;
    if (RECALC && !changed[i] && !changed[j]) return;
    const int64_t at = ((int64_t)s * n + i) * n * 4 + c;
    mutual[at] = j == i ? __builtin_inff() : (compat[at] + compat[(((int64_t)sj * n + j) * n + i) * 4 + s]) / 2.0f;
}

// Best buddies: the unique candidates (piece, side) that name each other.
__global__ void __launch_bounds__(THREADS) best_buddy2_kernel(const int* __restrict__ candidate, int n, int* __restrict__ best_buddy) {
    const int t = blockIdx.x * THREADS + threadIdx.x;
    if (t >= 4 * n) return;
    const int i = t / 4, s = t % 4, j = candidate[2 * t], sj = candidate[2 * t + 1];
    const bool mutual = j >= 0 && candidate[2 * (j * 4 + sj)] == i && candidate[2 * (j * 4 + sj) + 1] == s;
    best_buddy[2 * t] = mutual ? j : -1;
    best_buddy[2 * t + 1] = mutual ? sj : -1;
}

// The start-piece keys of type 1 on (piece, side) best buddies.
__global__ void __launch_bounds__(THREADS) start_keys2_kernel(const int* __restrict__ best_buddy, const float* __restrict__ mutual, int n,
                                                              int* __restrict__ start_count, float* __restrict__ start_total) {
    const int i = blockIdx.x * THREADS + threadIdx.x;
    if (i >= n) return;
    int count = 0;
    float total = 0.0f;
    for (int s = 0; s < 4; ++s) {
        const int j = best_buddy[2 * (i * 4 + s)], sj = best_buddy[2 * (i * 4 + s) + 1];
        if (j < 0) continue;
        count += 4;
        for (int t = 0; t < 4; ++t) count += best_buddy[2 * (j * 4 + t)] >= 0;
        total = total + mutual[(((int64_t)s * n + i) * n + j) * 4 + sj];
    }
    start_count[i] = count;
    start_total[i] = total;
}

// Slot scan of _get_next_piece_from_pool for type 2: the first maximum of M[side, p, q, sq] over unplaced pieces p ascending x open slots
// (q, sq) in list order x the piece's side 0..3, sq the unrotated side of the placed piece q that faces the slot.  Packed as in type 1.
__global__ void __launch_bounds__(THREADS) best_slot2_kernel(const float* __restrict__ mutual, int n, const int* __restrict__ placed,
                                                             const int* __restrict__ slot_piece, const int* __restrict__ slot_side, int slots,
                                                             unsigned long long* __restrict__ best) {
    const int64_t per_piece = (int64_t)slots * 4, total = (int64_t)n * per_piece;
    unsigned long long word = 0;
    for (int64_t lin = (int64_t)blockIdx.x * THREADS + threadIdx.x; lin < total; lin += (int64_t)gridDim.x * THREADS) {
        const int p = (int)(lin / per_piece), rem = (int)(lin % per_piece);
        const int k = rem >> 2, side = rem & 3;
        const int q = slot_piece[k];
        if (placed[p] || q < 0 || q >= n) continue;
        const float v = mutual[(((int64_t)side * n + p) * n + q) * 4 + (slot_side[k] & 3)];
        const unsigned long long w = ((unsigned long long)order_key(v) << 32) | (0xffffffffu - (uint32_t)lin);
        word = w > word ? w : word;
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        const unsigned long long o = __shfl_xor(word, off, 64);
        word = o > word ? o : word;
    }
    if (threadIdx.x % VITED_WAVE == 0 && word != 0) atomicMax(best, word);
}

// The solver's point lookups of M (solver.py:490, :630, :688) without a host copy of it: lookup r is (side, p, q) -> M[side, p, q]
// (type 1, WIDTH 3) or (side_p, p, q, side_q) -> M[side_p, p, q, side_q] (type 2, WIDTH 4).  The word moves as an integer, so every
// bit pattern arrives as it lies in M.  A lookup outside the tensor leaves its slot alone and flags bad.
template <int WIDTH>
__global__ void __launch_bounds__(VITED_WAVE) mutual_gather_kernel(const uint32_t* __restrict__ mutual, int n,
                                                                   const int* __restrict__ lookups, int64_t m,
                                                                   uint32_t* __restrict__ out, int* __restrict__ bad) {
    const int64_t r = (int64_t)blockIdx.x * VITED_WAVE + threadIdx.x;
    if (r >= m) return;
    const int* look = lookups + r * WIDTH;
    const int side = look[0], p = look[1], q = look[2], side_q = WIDTH == 4 ? look[3] : 0;
    if (side < 0 || side > 3 || p < 0 || p >= n || q < 0 || q >= n || side_q < 0 || side_q > 3) {
        atomicOr(bad, 1);
        return;
    }
    const int64_t at = ((int64_t)side * n + p) * n + q;
    out[r] = mutual[WIDTH == 4 ? at * 4 + side_q : at];
}

inline unsigned blocks_for(int64_t work) { return (unsigned)ceil_div64(work, THREADS); }

template <int WIDTH>
int launch_mutual_gather(const float* mutual, int64_t n, const int* lookups, int64_t m, float* out, int* bad, void* stream) {
    if (!mutual || !lookups || !out || !bad || m < 0 || n < 2 || n > MAX_PIECES) return VITED_ERR_BAD_ARG;
    if (m > (int64_t)INT32_MAX) return VITED_ERR_UNSUPPORTED;
    if (m == 0) return VITED_OK;
    hipLaunchKernelGGL(mutual_gather_kernel<WIDTH>, dim3((unsigned)ceil_div64(m, VITED_WAVE)), dim3(VITED_WAVE), 0,
                       static_cast<hipStream_t>(stream), reinterpret_cast<const uint32_t*>(mutual), (int)n, lookups, m,
                       reinterpret_cast<uint32_t*>(out), bad);
    return vited_check_launch();
}

}  // namespace

extern "C" int vited_puzzle_distances_from_logits(const float* logits, const int64_t* pi, const int64_t* pj, int64_t m, int64_t n, int* dq,
                                                  int* bad, void* stream) {
    if (!logits || !pi || !pj || !dq || !bad || m < 0 || n < 2 || n > MAX_PIECES) return VITED_ERR_BAD_ARG;
    if (m == 0) return VITED_OK;
    hipLaunchKernelGGL(distances_kernel, dim3(blocks_for(m)), dim3(THREADS), 0, static_cast<hipStream_t>(stream), logits, pi, pj, m,
                       (int)n, dq, bad);
    return vited_check_launch();
}

extern "C" int vited_puzzle_distances2_from_logits(const float* logits, const int64_t* pi, const int64_t* pjt, int64_t m, int64_t n, int* dq2,
                                                   int* bad, void* stream) {
    if (!logits || !pi || !pjt || !dq2 || !bad || m < 0 || n < 2 || n > MAX_PIECES) return VITED_ERR_BAD_ARG;
    if (m == 0) return VITED_OK;
    hipLaunchKernelGGL(distances2_kernel, dim3(blocks_for(m)), dim3(THREADS), 0, static_cast<hipStream_t>(stream), logits, pi, pjt, m,
                       (int)n, dq2, bad);
    return vited_check_launch();
}

extern "C" int vited_puzzle_compat_init(const int* dq, int64_t n, int64_t* min_d, int64_t* second_d, int* candidate, int* best_buddy,
                                        float* compat, float* mutual, int* start_count, float* start_total, int* start_order, void* stream) {
    if (!dq || !min_d || !second_d || !candidate || !best_buddy || !compat || !mutual || !start_count || !start_total || !start_order)
        return VITED_ERR_BAD_ARG;
    if (n < 2 || n > MAX_PIECES) return VITED_ERR_BAD_ARG;
    hipStream_t st = static_cast<hipStream_t>(stream);
    const int ni = (int)n;
    const dim3 grid2((unsigned)ceil_div64(n, THREADS), (unsigned)(4 * n));
    hipLaunchKernelGGL(min_second_kernel<false>, dim3((unsigned)ceil_div64(4 * n, ROWS_PER_BLOCK)), dim3(THREADS), 0, st, dq, ni,
                       (const int*)nullptr, min_d, second_d, candidate, (int*)nullptr);
    hipLaunchKernelGGL(compat_kernel<false>, grid2, dim3(THREADS), 0, st, dq, ni, (const int*)nullptr, (const int*)nullptr, second_d,
                       compat);
    hipLaunchKernelGGL(mutual_kernel<false>, grid2, dim3(THREADS), 0, st, compat, ni, (const int*)nullptr, mutual);
    hipLaunchKernelGGL(best_buddy_kernel, dim3(blocks_for(4 * n)), dim3(THREADS), 0, st, candidate, ni, best_buddy);
    hipLaunchKernelGGL(start_keys_kernel, dim3(blocks_for(n)), dim3(THREADS), 0, st, best_buddy, mutual, ni, start_count, start_total);
    hipLaunchKernelGGL(start_order_kernel, dim3(blocks_for(n)), dim3(THREADS), 0, st, start_count, start_total, ni, start_order);
    return vited_check_launch();
}

extern "C" int vited_puzzle_compat_recalc(const int* dq, int64_t n, const int* placed, int64_t* min_d, int64_t* second_d, float* compat,
                                          float* mutual, int* changed, void* stream) {
    if (!dq || !placed || !min_d || !second_d || !compat || !mutual || !changed || n < 2 || n > MAX_PIECES) return VITED_ERR_BAD_ARG;
    hipStream_t st = static_cast<hipStream_t>(stream);
    const int ni = (int)n;
    const dim3 grid2((unsigned)ceil_div64(n, THREADS), (unsigned)(4 * n));
    if (hipMemsetAsync(changed, 0, sizeof(int) * n, st) != hipSuccess) return VITED_ERR_LAUNCH;
    hipLaunchKernelGGL(min_second_kernel<true>, dim3((unsigned)ceil_div64(4 * n, ROWS_PER_BLOCK)), dim3(THREADS), 0, st, dq, ni, placed,
                       min_d, second_d, (int*)nullptr, changed);
    hipLaunchKernelGGL(compat_kernel<true>, grid2, dim3(THREADS), 0, st, dq, ni, placed, (const int*)changed, (const int64_t*)second_d,
                       compat);
    hipLaunchKernelGGL(mutual_kernel<true>, grid2, dim3(THREADS), 0, st, (const float*)compat, ni, (const int*)changed, mutual);
    return vited_check_launch();
}

extern "C" int vited_puzzle_best_slot(const float* mutual, int64_t n, const int* placed, const int* slot_piece, const int* slot_side,
                                      int64_t slots, int64_t* best, void* stream) {
    if (!mutual || !placed || !slot_piece || !slot_side || !best || n < 2 || n > MAX_PIECES || slots < 1) return VITED_ERR_BAD_ARG;
    if (n * slots > (int64_t)UINT32_MAX) return VITED_ERR_UNSUPPORTED;
    hipStream_t st = static_cast<hipStream_t>(stream);
    if (hipMemsetAsync(best, 0, sizeof(int64_t), st) != hipSuccess) return VITED_ERR_LAUNCH;
    const int64_t want = ceil_div64(n * slots, THREADS), blocks = want < 1024 ? want : 1024;
    hipLaunchKernelGGL(best_slot_kernel, dim3((unsigned)blocks), dim3(THREADS), 0, st, mutual, (int)n, placed, slot_piece, slot_side,
                       (int)slots, reinterpret_cast<unsigned long long*>(best));
    return vited_check_launch();
}

// ---- type 2 --------------------------------------------------------------------------------------------------------------------------
extern "C" int vited_puzzle_compat2_init(const int* dq2, int64_t n, int64_t* min_d, int64_t* second_d, int* min_count, int* candidate,
                                         int* best_buddy, float* compat, float* mutual, int* start_count, float* start_total,
                                         int* start_order, void* stream) {
    if (!dq2 || !min_d || !second_d || !min_count || !candidate || !best_buddy || !compat || !mutual || !start_count || !start_total ||
        !start_order)
        return VITED_ERR_BAD_ARG;
    if (n < 2 || n > MAX_PIECES || reinterpret_cast<uintptr_t>(dq2) % 16 != 0) return VITED_ERR_BAD_ARG;
    hipStream_t st = static_cast<hipStream_t>(stream);
    const int ni = (int)n;
    const dim3 grid2((unsigned)(4 * n), (unsigned)ceil_div64(4 * n, THREADS));
    hipLaunchKernelGGL(min_second2_kernel<false>, dim3((unsigned)ceil_div64(4 * n, ROWS_PER_BLOCK)), dim3(THREADS), 0, st, dq2, ni,
                       (const int*)nullptr, min_d, second_d, min_count, candidate, (int*)nullptr);
    hipLaunchKernelGGL(compat2_kernel<false>, grid2, dim3(THREADS), 0, st, dq2, ni, (const int*)nullptr, (const int*)nullptr,
                       (const int64_t*)second_d, compat);
    hipLaunchKernelGGL(mutual2_kernel<false>, grid2, dim3(THREADS), 0, st, (const float*)compat, ni, (const int*)nullptr, mutual);
    hipLaunchKernelGGL(best_buddy2_kernel, dim3(blocks_for(4 * n)), dim3(THREADS), 0, st, (const int*)candidate, ni, best_buddy);
    hipLaunchKernelGGL(start_keys2_kernel, dim3(blocks_for(n)), dim3(THREADS), 0, st, (const int*)best_buddy, (const float*)mutual, ni,
                       start_count, start_total);
    hipLaunchKernelGGL(start_order_kernel, dim3(blocks_for(n)), dim3(THREADS), 0, st, (const int*)start_count, (const float*)start_total,
                       ni, start_order);
    return vited_check_launch();
}

extern "C" int vited_puzzle_compat2_recalc(const int* dq2, int64_t n, const int* placed, int64_t* min_d, int64_t* second_d, float* compat,
                                           float* mutual, int* changed, void* stream) {
    if (!dq2 || !placed || !min_d || !second_d || !compat || !mutual || !changed || n < 2 || n > MAX_PIECES) return VITED_ERR_BAD_ARG;
    if (reinterpret_cast<uintptr_t>(dq2) % 16 != 0) return VITED_ERR_BAD_ARG;
    hipStream_t st = static_cast<hipStream_t>(stream);
    const int ni = (int)n;
    const dim3 grid2((unsigned)(4 * n), (unsigned)ceil_div64(4 * n, THREADS));
    if (hipMemsetAsync(changed, 0, sizeof(int) * n, st) != hipSuccess) return VITED_ERR_LAUNCH;
    hipLaunchKernelGGL(min_second2_kernel<true>, dim3((unsigned)ceil_div64(4 * n, ROWS_PER_BLOCK)), dim3(THREADS), 0, st, dq2, ni, placed,
                       min_d, second_d, (int*)nullptr, (int*)nullptr, changed);
    hipLaunchKernelGGL(compat2_kernel<true>, grid2, dim3(THREADS), 0, st, dq2, ni, placed, (const int*)changed, (const int64_t*)second_d,
                       compat);
    hipLaunchKernelGGL(mutual2_kernel<true>, grid2, dim3(THREADS), 0, st, (const float*)compat, ni, (const int*)changed, mutual);
    return vited_check_launch();
}

extern "C" int vited_puzzle_best_slot2(const float* mutual, int64_t n, const int* placed, const int* slot_piece, const int* slot_side,
                                       int64_t slots, int64_t* best, void* stream) {
    if (!mutual || !placed || !slot_piece || !slot_side || !best || n < 2 || n > MAX_PIECES || slots < 1) return VITED_ERR_BAD_ARG;
    if (slots > (int64_t)UINT32_MAX || 4 * n * slots > (int64_t)UINT32_MAX) return VITED_ERR_UNSUPPORTED;
    hipStream_t st = static_cast<hipStream_t>(stream);
    if (hipMemsetAsync(best, 0, sizeof(int64_t), st) != hipSuccess) return VITED_ERR_LAUNCH;
    const int64_t want = ceil_div64(4 * n * slots, THREADS), blocks = want < 1024 ? want : 1024;
    hipLaunchKernelGGL(best_slot2_kernel, dim3((unsigned)blocks), dim3(THREADS), 0, st, mutual, (int)n, placed, slot_piece, slot_side,
                       (int)slots, reinterpret_cast<unsigned long long*>(best));
    return vited_check_launch();
}

// ---- point lookups of M for the placement loop (mixed bags and unknown dimensions) ----------------------------------
extern "C" int vited_puzzle_mutual_gather(const float* mutual, int64_t n, const int* lookups, int64_t m, float* out, int* bad,
                                          void* stream) {
    return launch_mutual_gather<3>(mutual, n, lookups, m, out, bad, stream);
}

extern "C" int vited_puzzle_mutual_gather2(const float* mutual, int64_t n, const int* lookups, int64_t m, float* out, int* bad,
                                           void* stream) {
    return launch_mutual_gather<4>(mutual, n, lookups, m, out, bad, stream);
}
