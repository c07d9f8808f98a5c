// Row-sparse gradient of the term-embedding table and its lazy Adam step.
//
// A training batch reads the table through two gathers: x = features[_id] (one row per batch node, n_a of them) and the distinct query
// rows (n_b of them).  Backward leaves one gradient row per OCCURRENCE, d_a [n_a][d] and d_b [n_b][d]; the same table row occurs many
// times (parents, hubs, the pseudo leaf).  Two entry points turn that into an updated table:
//
//   txe_rowgrad_group      the occurrences grouped by table row.  key = the row id (an id outside [0, n_rows) gets the key n_rows: it
//                          sorts behind every row and is never used as an address), value = the occurrence index (a's occurrences are
//                          0 .. n_a-1, b's are n_a .. n_a+n_b-1); ONE stable radix sort over the ceil(log2(n_rows + 1)) key bits
//                          (rocPRIM through hipCUB, as txe_graph.hip: index preparation), then the positions at which the sorted key
//                          changes (hipcub::DeviceSelect::If over a counting iterator).  Stable: within a row the occurrences ascend,
//                          all of a's before b's.
//   txe_sparse_adam_rows   ONE launch.  A segment (= the occurrences of one row) belongs to one wave, or, when it is long, to the 16
//                          waves of one workgroup; the wave that holds the row's gradient sum applies txe_adam_step's update
//                          (txe_adam.h: the same expression, the same fma placement) to that row of weight / exp_avg / exp_avg_sq
//                          [/ max_exp_avg_sq].  Rows that do not occur are neither read nor written.  One writer per table element,
//                          no floating-point atomics: two calls on the same inputs give the same bytes.
//
// THE SUMMATION ORDER of a segment of L gradient rows g_0 .. g_{L-1} (grouped order), per column, in fp32 -- a function of L alone:
//   L <= 64:  s = g_0;  s = s + g_k  for k = 1 .. L-1                                  (one wave, left to right)
//   L >  64:  c = ceil(L / 16); slice j = 0 .. ceil(L / c) - 1 holds g_{jc} .. g_{min(L, (j+1)c) - 1} and is summed as above into p_j
//             (wave j of the workgroup); s = p_0;  s = s + p_j  for j = 1 .. ceil(L / c) - 1   (wave 0, through LDS, left to right)
// feature_table.host_row_sums restates it.  The loads of a slice are issued eight rows at a time (four with 16-byte loads: the index loads, then the row loads
// with no branch between them); the additions keep the order above.
//
// Geometry.  A workgroup of 1,024 threads walks tiles of 16 consecutive segments: wave w sums and updates segment 16 t + w when it has
// at most 64 occurrences; the tile's longer segments are then taken one after the other by all 16 waves.  A wave covers 64 V columns
// per pass, V = 4, 2 or 1 floats per lane: the widest access that every pointer and pitch of the call allows (d = 250 at pitch 250 has
// 8-byte aligned rows: V = 2); the columns of a last partial vector are read and written element by element.
#include <hipcub/hipcub.hpp>

#include <mutex>
#include <unordered_map>

#include "txe_common.h"
#include "txe_adam.h"

namespace txe {

constexpr int RG_WAVES = 16;                    // waves per workgroup = segments per tile = slices of a long segment
constexpr int RG_THREADS = RG_WAVES * TXE_WAVE;
constexpr int RG_SPLIT = 64;                    // a segment longer than this is split over the workgroup's waves
constexpr int RG_UNROLL = 8;                    // gradient rows in flight per lane (four with 16-byte loads)
constexpr int RG_MAX_GRID = 512;                // two workgroups per CU hold every wave slot of the chip

struct RowgradArgs {
    float* w; float* m; float* v; float* x;     // the table and its moments, row pitch ld_w (x = max_exp_avg_sq, or v without AMSGrad)
    long long ld_w;
    int n_rows, d;
    const float* ga; long long ld_a; int n_a;
    const float* gb; long long ld_b;
    int n;                                      // n_a + n_b
    const int* n_seg; const int* rows; const int* occ; const int* heads;        // the grouping (the workspace of txe_rowgrad_group)
    const unsigned char* trainable;
    const long long* first_bad;
};

static inline size_t rg_align(size_t x) { return (x + 255) / 256 * 256; }

// key[i] = the row of occurrence i, or n_rows for an id outside the table; val[i] = i
__global__ void rowgrad_keys_kernel(const int* __restrict__ ids_a, int n_a, const int* __restrict__ ids_b, int n_b, int n_rows,
                                    int* __restrict__ keys, int* __restrict__ vals) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n_a + n_b) return;
    const int id = i < n_a ? ids_a[i] : ids_b[i - n_a];
    keys[i] = (id >= 0 && id < n_rows) ? id : n_rows;
    vals[i] = i;
}

// position i opens a segment of the sorted keys
struct RowgradHead {
    const int* keys;
    __host__ __device__ bool operator()(const int& i) const { return i == 0 || keys[i] != keys[i - 1]; }
};

// bytes of library scratch for n occurrences (the larger of the sort's and the select's; a function of n alone): the two size queries
// run once per n -- a step asks the same n several times, from the host, in a path that is latency-bound -- and a query that fails is
// an error (TXE_ERR_LAUNCH; txe_rowgrad_ws_bytes: 0), not a silent size of 0
static bool rowgrad_temp_bytes(int n, size_t* out) {
    static std::mutex mu;
    static std::unordered_map<int, size_t> known;
    const int m = n > 0 ? n : 1;
    std::lock_guard<std::mutex> lock(mu);
    const auto it = known.find(m);
    if (it != known.end()) { *out = it->second; return true; }
    // (hipErrorNoDevice: a host without a GPU, where only the argument checks can run -- the scratch counts as 0 there, and a size is
    //  good for the machine it was asked on.  Any other error is a failed query.)
    size_t a = 0, b = 0;
    const hipError_t ea = hipcub::DeviceRadixSort::SortPairs(nullptr, a, (const int*)nullptr, (int*)nullptr, (const int*)nullptr, (int*)nullptr, m);
    const hipError_t eb = hipcub::DeviceSelect::If(nullptr, b, hipcub::CountingInputIterator<int>(0), (int*)nullptr, (int*)nullptr, m,
                                                   RowgradHead{nullptr});
    if (ea != hipSuccess || eb != hipSuccess) (void)hipGetLastError();      // (not for the next launch check to find)
    if ((ea != hipSuccess && ea != hipErrorNoDevice) || (eb != hipSuccess && eb != hipErrorNoDevice)) return false;
    if (ea != hipSuccess) a = 0;
    if (eb != hipSuccess) b = 0;
    if (known.size() > 256) known.clear();
    *out = known[m] = a > b ? a : b;
    return true;
}

// the workspace: [n_seg + padding: 256 bytes | rows: e | occ: e | heads: e | unsorted keys: e | unsorted values: e | library scratch]
struct RowgradWs {
    int* n_seg; int* rows; int* occ; int* heads; int* keys_in; int* vals_in; void* temp; size_t temp_bytes, total;
};
// the layout for n occurrences over the buffer ws (which may be null when only `total` is wanted); false: a size query failed
static bool rowgrad_ws(void* ws, long long n, RowgradWs* w) {
    const size_t e = rg_align(4 * (size_t)(n > 0 ? n : 1));
    char* b = (char*)ws;
    w->n_seg = (int*)b;
    w->rows = (int*)(b + 256);
    w->occ = (int*)(b + 256 + e);
    w->heads = (int*)(b + 256 + 2 * e);
    w->keys_in = (int*)(b + 256 + 3 * e);
    w->vals_in = (int*)(b + 256 + 4 * e);
    w->temp = b + 256 + 5 * e;
    if (!rowgrad_temp_bytes((int)n, &w->temp_bytes)) return false;
    w->total = 256 + 5 * e + rg_align(w->temp_bytes);
    return true;
}

template <int V> struct RgVec { float e[V]; };

// a whole vector of V floats (the pointer is V-float aligned by the launcher's choice of V) / the nv < V columns of a row's last, partial
// vector element by element.  The callers branch ONCE on nv == V and then issue their loads back to back: a branch inside every load
// would put a wait between two loads and expose each one's latency.
template <int V>
__device__ __forceinline__ RgVec<V> rg_load_full(const float* __restrict__ p) {
    RgVec<V> r;
    if constexpr (V == 4) {
        const float4 t = *reinterpret_cast<const float4*>(p);
        r.e[0] = t.x; r.e[1] = t.y; r.e[2] = t.z; r.e[3] = t.w;
    } else if constexpr (V == 2) {
        const float2 t = *reinterpret_cast<const float2*>(p);
        r.e[0] = t.x; r.e[1] = t.y;
    } else {
        r.e[0] = p[0];
    }
    return r;
}
template <int V>
__device__ __forceinline__ RgVec<V> rg_load_tail(const float* __restrict__ p, int nv) {
    RgVec<V> r;
#pragma unroll
    for (int k = 0; k < V; ++k) r.e[k] = k < nv ? p[k] : 0.f;
    return r;
}
template <int V, bool FULL>
__device__ __forceinline__ RgVec<V> rg_load(const float* __restrict__ p, int nv) {
    if constexpr (FULL) return rg_load_full<V>(p);
    else return rg_load_tail<V>(p, nv);
}

template <int V, bool FULL>
__device__ __forceinline__ void rg_store(float* __restrict__ p, const RgVec<V>& r, int nv) {
    if constexpr (FULL) {
        if constexpr (V == 4) *reinterpret_cast<float4*>(p) = make_float4(r.e[0], r.e[1], r.e[2], r.e[3]);
        else if constexpr (V == 2) *reinterpret_cast<float2*>(p) = make_float2(r.e[0], r.e[1]);
        else p[0] = r.e[0];
    } else {
#pragma unroll
        for (int k = 0; k < V; ++k)
            if (k < nv) p[k] = r.e[k];
    }
}

// the gradient row of occurrence o (0 <= o < n by construction: the values of the sort are an iota)
__device__ __forceinline__ const float* rg_grad_row(const RowgradArgs& A, int o) {
    return o < A.n_a ? A.ga + (long long)o * A.ld_a : A.gb + (long long)(o - A.n_a) * A.ld_b;
}

// s = g_beg; s = s + g_k for k = beg+1 .. end-1 (sorted positions), columns col .. col+nv-1; beg < end.  Per round: RG_UNROLL independent
// index loads, then as many independent row loads, then the additions in order.
template <int V, bool FULL>
__device__ __forceinline__ RgVec<V> rg_sum_as(const RowgradArgs& A, int beg, int end, int col, int nv) {
    constexpr int U = V == 4 ? RG_UNROLL / 2 : RG_UNROLL;     // (16-byte loads: half as many keep the same bytes in flight, and the registers)
    RgVec<V> s = rg_load<V, FULL>(rg_grad_row(A, A.occ[beg]) + col, nv);
    int k = beg + 1;
    for (; k + U <= end; k += U) {
        int o[U];
#pragma unroll
        for (int u = 0; u < U; ++u) o[u] = A.occ[k + u];
        RgVec<V> t[U];
#pragma unroll
        for (int u = 0; u < U; ++u) t[u] = rg_load<V, FULL>(rg_grad_row(A, o[u]) + col, nv);
#pragma unroll
        for (int u = 0; u < U; ++u)
#pragma unroll
            for (int j = 0; j < V; ++j) s.e[j] = s.e[j] + t[u].e[j];
    }
    for (; k < end; ++k) {
        const RgVec<V> t = rg_load<V, FULL>(rg_grad_row(A, A.occ[k]) + col, nv);
#pragma unroll
        for (int j = 0; j < V; ++j) s.e[j] = s.e[j] + t.e[j];
    }
    return s;
}
template <int V>
__device__ __forceinline__ RgVec<V> rg_sum(const RowgradArgs& A, int beg, int end, int col, int nv) {
    return nv == V ? rg_sum_as<V, true>(A, beg, end, col, nv) : rg_sum_as<V, false>(A, beg, end, col, nv);
}

// the state of columns col .. col+nv-1 of one table row, loaded before the gradient sum is formed and stored after the update
template <int V, bool AMS>
struct RgRowState {
    RgVec<V> p, m, v, x;
    template <bool FULL>
    __device__ __forceinline__ void load_as(const RowgradArgs& A, long long at, int nv) {
        p = rg_load<V, FULL>(A.w + at, nv);
        m = rg_load<V, FULL>(A.m + at, nv);
        v = rg_load<V, FULL>(A.v + at, nv);
        if (AMS) x = rg_load<V, FULL>(A.x + at, nv);
    }
    __device__ __forceinline__ void load(const RowgradArgs& A, long long at, int nv) {
        if (nv == V) load_as<true>(A, at, nv);
        else load_as<false>(A, at, nv);
    }
    template <bool FULL>
    __device__ __forceinline__ void store_as(const RowgradArgs& A, long long at, int nv) {
        rg_store<V, FULL>(A.w + at, p, nv);
        rg_store<V, FULL>(A.m + at, m, nv);
        rg_store<V, FULL>(A.v + at, v, nv);
        if (AMS) rg_store<V, FULL>(A.x + at, x, nv);
    }
    __device__ __forceinline__ void step_and_store(const RowgradArgs& A, const AdamScalars& c, long long at, int nv, const RgVec<V>& g) {
#pragma unroll
        for (int j = 0; j < V; ++j) {
            float xm = AMS ? x.e[j] : 0.f;
            adam_one<false>(p.e[j], g.e[j], m.e[j], v.e[j], xm, AMS, c, 1.f);
            if (AMS) x.e[j] = xm;
        }
        if (nv == V) store_as<true>(A, at, nv);
        else store_as<false>(A, at, nv);
    }
};

template <int V, bool AMS>
__global__ __launch_bounds__(RG_THREADS) void sparse_adam_rows_kernel(RowgradArgs A, AdamScalars c) {
    if (A.first_bad && A.first_bad[0] >= 0) return;         // frozen: nothing is loaded, nothing is stored
    __shared__ float part[RG_WAVES][TXE_WAVE * V];
    __shared__ int sh_beg[RG_WAVES], sh_end[RG_WAVES], sh_row[RG_WAVES];
    const int lane = threadIdx.x & (TXE_WAVE - 1), wave = threadIdx.x / TXE_WAVE;
    const int n_seg = A.n_seg[0];                           // (the same value in every thread: the tile loop and its barriers are uniform)
    for (int s0 = blockIdx.x * RG_WAVES; s0 < n_seg; s0 += gridDim.x * RG_WAVES) {
        const int s = s0 + wave;
        int beg = 0, end = 0, row = -1;
        if (s < n_seg) {
            beg = A.heads[s];
            end = (s + 1 < n_seg) ? A.heads[s + 1] : A.n;
            row = A.rows[beg];
            if (row >= A.n_rows || (A.trainable && A.trainable[row] == 0)) row = -1;     // the dropped ids' segment; a frozen row
        }
        const bool is_long = row >= 0 && end - beg > RG_SPLIT;
        if (row >= 0 && !is_long) {
            for (int col = lane * V; col < A.d; col += TXE_WAVE * V) {
                const int nv = A.d - col < V ? A.d - col : V;
                const long long at = (long long)row * A.ld_w + col;
                RgRowState<V, AMS> st;
                st.load(A, at, nv);
                const RgVec<V> g = rg_sum<V>(A, beg, end, col, nv);
                st.step_and_store(A, c, at, nv, g);
            }
        }
        if (lane == 0) { sh_beg[wave] = beg; sh_end[wave] = end; sh_row[wave] = is_long ? row : -1; }
        __syncthreads();
        for (int k = 0; k < RG_WAVES; ++k) {
            const int lrow = sh_row[k];
            if (lrow < 0) continue;                         // (uniform over the workgroup)
            const int lbeg = sh_beg[k], L = sh_end[k] - lbeg;
            const int per = (L + RG_WAVES - 1) / RG_WAVES, n_slices = (L + per - 1) / per;
            const int b0 = lbeg + wave * per, b1 = (b0 + per < lbeg + L) ? b0 + per : lbeg + L;
            for (int col0 = 0; col0 < A.d; col0 += TXE_WAVE * V) {
                const int col = col0 + lane * V;
                const bool live = col < A.d;
                const int nv = A.d - col < V ? A.d - col : V;
                const long long at = (long long)lrow * A.ld_w + col;
                RgRowState<V, AMS> st;
                if (wave == 0 && live) st.load(A, at, nv);
                if (wave < n_slices && live) {
                    const RgVec<V> pj = rg_sum<V>(A, b0, b1, col, nv);
#pragma unroll
                    for (int j = 0; j < V; ++j) part[wave][lane * V + j] = pj.e[j];
                }
                __syncthreads();
                if (wave == 0 && live) {
                    RgVec<V> g;
#pragma unroll
                    for (int j = 0; j < V; ++j) g.e[j] = part[0][lane * V + j];
                    for (int w = 1; w < n_slices; ++w)
#pragma unroll
                        for (int j = 0; j < V; ++j) g.e[j] = g.e[j] + part[w][lane * V + j];
                    st.step_and_store(A, c, at, nv, g);
                }
                __syncthreads();
            }
        }
        __syncthreads();                                    // sh_* are rewritten by the next tile
    }
}

// dst[u] = src[run_off[u]] + src[run_off[u] + 1] + ... (left to right; an empty run gives 0): the backward of a query row repeated over
// the pairs of its run (ops.RepeatedRows.dense), one workgroup per run, one column per thread.  Offsets are clamped to [0, G].
__global__ __launch_bounds__(256) void rows_run_sum_kernel(const float* __restrict__ src, long long ld_s, const int* __restrict__ run_off, int G,
                                                           int r, float* __restrict__ dst, long long ld_d) {
    const int u = blockIdx.x;
    int beg = run_off[u], end = run_off[u + 1];
    beg = beg < 0 ? 0 : (beg > G ? G : beg);
    end = end < beg ? beg : (end > G ? G : end);
    for (int col = threadIdx.x; col < r; col += blockDim.x) {
        float s = 0.f;
        if (beg < end) {
            s = src[(long long)beg * ld_s + col];
            for (int i = beg + 1; i < end; ++i) s = s + src[(long long)i * ld_s + col];
        }
        dst[(long long)u * ld_d + col] = s;
    }
}

template <int V>
static void launch_sparse_adam(bool ams, int grid, hipStream_t s, const RowgradArgs& A, const AdamScalars& c) {
    if (ams) hipLaunchKernelGGL((sparse_adam_rows_kernel<V, true>), dim3(grid), dim3(RG_THREADS), 0, s, A, c);
    else hipLaunchKernelGGL((sparse_adam_rows_kernel<V, false>), dim3(grid), dim3(RG_THREADS), 0, s, A, c);
}

}  // namespace txe

using namespace txe;

extern "C" {

// bytes of the workspace that txe_rowgrad_group fills and txe_sparse_adam_rows reads, for n_a + n_b occurrences (negative counts count
// as 0); 0 when the sum does not fit an int or the library's size query fails
size_t txe_rowgrad_ws_bytes(int n_a, int n_b) {
    const long long n = (long long)(n_a > 0 ? n_a : 0) + (n_b > 0 ? n_b : 0);
    if (n > 0x7fffffffLL) return 0;
    RowgradWs w;
    return rowgrad_ws(nullptr, n, &w) ? w.total : 0;
}

// Group the occurrences ids_a [n_a] and ids_b [n_b] (int32, DEVICE) by table row into ws (include/txe.h has the layout).
int txe_rowgrad_group(const int* ids_a, int n_a, const int* ids_b, int n_b, int n_rows, void* ws, size_t ws_bytes, void* stream) {
    if (n_a < 0 || n_b < 0 || n_rows < 0 || (n_a > 0 && !ids_a) || (n_b > 0 && !ids_b)) return TXE_ERR_ARG;
    const long long n = (long long)n_a + n_b;
    if (n > 0x7fffffffLL) return TXE_ERR_ARG;
    if (n == 0) return TXE_OK;                              // nothing to group, and txe_sparse_adam_rows launches nothing either
    RowgradWs w;                                            // the layout, once per call
    if (!rowgrad_ws(ws, n, &w)) return TXE_ERR_LAUNCH;
    if (!ws || ws_bytes < w.total) return TXE_ERR_ARG;
    hipStream_t s = (hipStream_t)stream;
    int bits = 1;
    while ((1ll << bits) < (long long)n_rows + 1) ++bits;
    ProfScope prof("rowgrad_group", s, 8.0 * n, 1);
    hipLaunchKernelGGL(rowgrad_keys_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, ids_a, n_a, ids_b, n_b, n_rows, w.keys_in,
                       w.vals_in);
    size_t tb = w.temp_bytes;
    if (hipcub::DeviceRadixSort::SortPairs(w.temp, tb, (const int*)w.keys_in, w.rows, (const int*)w.vals_in, w.occ, (int)n, 0, bits, s) !=
        hipSuccess)
        return TXE_ERR_LAUNCH;
    tb = w.temp_bytes;
    if (hipcub::DeviceSelect::If(w.temp, tb, hipcub::CountingInputIterator<int>(0), w.heads, w.n_seg, (int)n, RowgradHead{w.rows}, s) !=
        hipSuccess)
        return TXE_ERR_LAUNCH;
    TXE_CHECK_LAUNCH();
    return TXE_OK;
}

// dst [U][ld_dst >= r]: row u = the sum of rows run_off[u] .. run_off[u+1]-1 of src [G][ld_src >= r], left to right (include/txe.h)
int txe_rows_run_sum(const float* src, long long ld_src, const int* run_off, int U, int G, int r, float* dst, long long ld_dst, void* stream) {
    if (U < 0 || G < 0 || r < 1 || ld_src < r || ld_dst < r) return TXE_ERR_ARG;
    if (U > 0 && (!run_off || !dst || (G > 0 && !src))) return TXE_ERR_ARG;
    if (U == 0) return TXE_OK;
    ProfScope prof("rows_run_sum_kernel", (hipStream_t)stream, 4.0 * ((double)G + U) * r, 1);
    hipLaunchKernelGGL(rows_run_sum_kernel, dim3(U), dim3(256), 0, (hipStream_t)stream, src, ld_src, run_off, G, r, dst, ld_dst);
    TXE_CHECK_LAUNCH();
    return TXE_OK;
}

// The lazy Adam step over the rows that txe_rowgrad_group found (include/txe.h).
int txe_sparse_adam_rows(float* weight, float* exp_avg, float* exp_avg_sq, float* max_exp_avg_sq, long long ld_w, int n_rows, int d,
                         const float* d_a, long long ld_a, int n_a, const float* d_b, long long ld_b, int n_b, const void* ws,
                         size_t ws_bytes, const unsigned char* trainable, double lr, double beta1, double beta2, double eps,
                         long long step, const long long* first_bad, void* stream) {
    if (n_a < 0 || n_b < 0 || n_rows < 0 || d < 1 || ld_w < d || step < 1) return TXE_ERR_ARG;
    if (!(beta1 >= 0.0 && beta1 < 1.0 && beta2 >= 0.0 && beta2 < 1.0)) return TXE_ERR_ARG;
    if ((n_a > 0 && (!d_a || ld_a < d)) || (n_b > 0 && (!d_b || ld_b < d))) return TXE_ERR_ARG;
    const long long n = (long long)n_a + n_b;
    if (n > 0x7fffffffLL) return TXE_ERR_ARG;
    if (n_rows > 0 && (!weight || !exp_avg || !exp_avg_sq)) return TXE_ERR_ARG;
    RowgradWs w;                                            // the layout, once per call
    if (n > 0) {
        if (!rowgrad_ws(const_cast<void*>(ws), n, &w)) return TXE_ERR_LAUNCH;
        if (!ws || ws_bytes < w.total) return TXE_ERR_ARG;
    }
    if (n == 0 || n_rows == 0) return TXE_OK;               // no occurrence, or none that is inside the table
    hipStream_t s = (hipStream_t)stream;
    const bool ams = max_exp_avg_sq != nullptr;
    RowgradArgs A;
    A.w = weight; A.m = exp_avg; A.v = exp_avg_sq; A.x = ams ? max_exp_avg_sq : exp_avg_sq;
    A.ld_w = ld_w; A.n_rows = n_rows; A.d = d;
    A.ga = d_a; A.ld_a = n_a > 0 ? ld_a : d; A.n_a = n_a;
    A.gb = d_b; A.ld_b = n_b > 0 ? ld_b : d;
    A.n = (int)n;
    A.n_seg = w.n_seg; A.rows = w.rows; A.occ = w.occ; A.heads = w.heads;
    A.trainable = trainable; A.first_bad = first_bad;
    const AdamScalars c = adam_scalars(lr, beta1, beta2, eps, 0.0, step);
    // the widest access every row start allows: all bases and all pitches multiples of V floats
    uintptr_t bases = (uintptr_t)weight | (uintptr_t)exp_avg | (uintptr_t)exp_avg_sq | (uintptr_t)max_exp_avg_sq;
    long long pitches = ld_w;
    if (n_a > 0) { bases |= (uintptr_t)d_a; pitches |= ld_a; }
    if (n_b > 0) { bases |= (uintptr_t)d_b; pitches |= ld_b; }
    const int V = ((bases & 15) == 0 && (pitches & 3) == 0) ? 4 : (((bases & 7) == 0 && (pitches & 1) == 0) ? 2 : 1);
    const long long max_seg = n < (long long)n_rows + 1 ? n : (long long)n_rows + 1;
    const long long tiles = (max_seg + RG_WAVES - 1) / RG_WAVES;
    const int grid = (int)(tiles < RG_MAX_GRID ? tiles : RG_MAX_GRID);
    ProfScope prof(ams ? "sparse_adam_rows_kernel<ams>" : "sparse_adam_rows_kernel", s, 4.0 * (double)n * d, 1);   // the gradient rows read
    if (V == 4) launch_sparse_adam<4>(ams, grid, s, A, c);
    else if (V == 2) launch_sparse_adam<2>(ams, grid, s, A, c);
    else launch_sparse_adam<1>(ams, grid, s, A, c);
    TXE_CHECK_LAUNCH();
    return TXE_OK;
}

}  // extern "C"
