// The per-step device log of the training loop (trainer/trainer.py:63-65 reads `loss.item()` back every step to log it and to add it to
// the epoch's total; here one launch between backward and the optimizer records the step on the device and the host reads once per
// epoch): the loss, the squared L2 norm of all gradients, the running loss sum, and the first step whose loss or gradients are not finite.
// The gradients (1.76 M floats on the bench model) are a read-once HBM stream: one workgroup per 4,096 consecutive elements of one
// tensor, cut as txe_optim.hip cuts its table, 16-byte loads, fp64 accumulation.  Reduction order, fixed: a thread adds its 16 squares in
// element order, the 64 lanes of a wave fold by halves (lane l += lane l + 32, 16, ... 1), the four waves add in wave order; the
// workgroup that draws the last ticket then adds the workgroups' partials -- thread t its run of consecutive partials in index order,
// the threads folded like the lanes above.  No floating-point atomic: the result does not depend on which workgroup finishes when.
#include "txe_common.h"

#include <math.h>

namespace txe {

constexpr int LOG_MAX_T = 48;                       // tensors per launch (kernel-argument table)
constexpr int LOG_CHUNK = TXE_STEP_LOG_CHUNK;       // elements per workgroup
constexpr int LOG_THREADS = 256;
constexpr size_t LOG_TICKET_BYTES = 16;             // ws = [ticket, padded to 16 bytes | one fp64 partial per workgroup]
static_assert(LOG_CHUNK == 16 * LOG_THREADS, "a thread owns four float4 of its chunk");

struct LogTable {
    const float* g[LOG_MAX_T];
    long long n[LOG_MAX_T];
    int first_chunk[LOG_MAX_T + 1];     // relative to the launch's first workgroup
    int count;
};

struct LogOut {
    const float* loss;
    float* loss_log;
    double* gnorm2_log;
    double* acc;
    long long* first_bad;
    long long step;
};

// the total of the workgroup in thread 0 (every thread must call)
__device__ __forceinline__ double block_sum(double v, double* s_wave) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o, 64);
    if ((threadIdx.x & 63) == 0) s_wave[threadIdx.x >> 6] = v;
    __syncthreads();
    return ((s_wave[0] + s_wave[1]) + s_wave[2]) + s_wave[3];
}

__device__ __forceinline__ double sq4(double a, const float4 x) {
    a += (double)x.x * (double)x.x;
    a += (double)x.y * (double)x.y;
    a += (double)x.z * (double)x.z;
    a += (double)x.w * (double)x.w;
    return a;
}

// grid: the launch's chunks (one workgroup even when there are none).  Workgroup b owns partial[chunk_base + b]; n_partials counts the
// workgroups of ALL launches of the step, so the last ticket is drawn when every partial of the step has been published.
__global__ __launch_bounds__(LOG_THREADS) void step_log_kernel(LogTable T, LogOut O, unsigned* __restrict__ ticket,
                                                                unsigned long long* __restrict__ partial, int chunk_base, int n_partials) {
    __shared__ double s_wave[LOG_THREADS / 64];
    __shared__ int s_last;
    double a = 0.0;
    if (T.count > 0) {
        int t = 0;
#pragma unroll 1
        while (t + 1 < T.count && (int)blockIdx.x >= T.first_chunk[t + 1]) ++t;
        const long long n = T.n[t];
        const float* __restrict__ G = T.g[t];
        const long long c0 = (long long)((int)blockIdx.x - T.first_chunk[t]) * LOG_CHUNK;
        if (c0 + LOG_CHUNK <= n && (((uintptr_t)G) & 15) == 0) {          // a whole, aligned chunk (uniform over the workgroup)
            const float4* __restrict__ G4 = reinterpret_cast<const float4*>(G + c0);
            const float4 x0 = G4[threadIdx.x], x1 = G4[threadIdx.x + LOG_THREADS], x2 = G4[threadIdx.x + 2 * LOG_THREADS],
                         x3 = G4[threadIdx.x + 3 * LOG_THREADS];
            a = sq4(sq4(sq4(sq4(a, x0), x1), x2), x3);
        } else {                                                            // a tensor's tail, or a view that is not 16-byte aligned
            // every load is issued (from a clamped index) before the first square: a load under `i < n` would be waited for one by one
            float x[16];
#pragma unroll
            for (int j = 0; j < 4; ++j)
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    const long long i = c0 + 4 * ((long long)j * LOG_THREADS + threadIdx.x) + e;
                    const float v = G[i < n ? i : n - 1];
                    x[4 * j + e] = i < n ? v : 0.f;
                }
#pragma unroll
            for (int k = 0; k < 16; ++k) a += (double)x[k] * (double)x[k];
        }
    }
    const double mine = block_sum(a, s_wave);
    if (threadIdx.x == 0) {
        // publish: the partial as an agent-scope store, then the ticket as an agent-scope acquire-release add by the SAME thread -- the
        // add that draws the last ticket has every other workgroup's partial before it (C++ memory model; no fence to get wrong)
        __hip_atomic_store(partial + chunk_base + blockIdx.x, (unsigned long long)__double_as_longlong(mine), __ATOMIC_RELAXED,
                           __HIP_MEMORY_SCOPE_AGENT);
        const unsigned drawn = __hip_atomic_fetch_add(ticket, 1u, __ATOMIC_ACQ_REL, __HIP_MEMORY_SCOPE_AGENT);
        s_last = drawn == (unsigned)(n_partials - 1);
    }
    __syncthreads();
    if (!s_last) return;
    // the last workgroup: thread t adds partials [t * per, (t + 1) * per) in index order (agent-scope loads: they do not come from this
    // CU's L1, whichever thread of the workgroup did the acquire)
    const int per = (n_partials + LOG_THREADS - 1) / LOG_THREADS;
    double v = 0.0;
    for (long long i = (long long)threadIdx.x * per; i < n_partials && i < ((long long)threadIdx.x + 1) * per; ++i)
        v += __longlong_as_double((long long)__hip_atomic_load(partial + i, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT));
    __syncthreads();                                                        // (s_wave is read by thread 0 above, rewritten below)
    const double total = block_sum(v, s_wave);
    if (threadIdx.x == 0) {
        const float loss = O.loss[0];
        O.loss_log[O.step] = loss;
        O.gnorm2_log[O.step] = total;
        O.acc[0] += (double)loss;                  // steps are ordered on one stream: plain read-modify-write
        O.acc[1] += 1.0;
        // squares are >= 0 and 2^31 chunks of 4,096 of them stay below 1e91: the fp64 sum is finite exactly when every element is
        if (!(isfinite(loss) && isfinite(total)) && O.first_bad[0] < 0) O.first_bad[0] = O.step;
        __hip_atomic_store(ticket, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);      // ready for the next step
    }
}

}  // namespace txe

using namespace txe;

extern "C" {

size_t txe_step_log_ws_bytes(int n_chunks) {
    return LOG_TICKET_BYTES + sizeof(double) * (size_t)(n_chunks > 1 ? n_chunks : 1);
}

int txe_step_log(const float* loss, int n_tensors, const float* const* grads, const long long* numel, long long step, long long capacity,
                 float* loss_log, double* gnorm2_log, double* acc, long long* first_bad, void* ws, size_t ws_bytes, void* stream) {
    if (!loss || !loss_log || !gnorm2_log || !acc || !first_bad || !ws || n_tensors < 0 || step < 0 || step >= capacity) return TXE_ERR_ARG;
    if (n_tensors > 0 && (!grads || !numel)) return TXE_ERR_ARG;
    if (((uintptr_t)ws & 15) != 0) return TXE_ERR_ARG;
    long long chunks = 0;
    for (int t = 0; t < n_tensors; ++t) {            // the whole table is checked before the first launch
        if (numel[t] < 0 || (numel[t] > 0 && !grads[t])) return TXE_ERR_ARG;
        chunks += (numel[t] + LOG_CHUNK - 1) / LOG_CHUNK;
        if (chunks > 0x7fffffffLL) return TXE_ERR_ARG;
    }
    if (ws_bytes < txe_step_log_ws_bytes((int)chunks)) return TXE_ERR_WORKSPACE;
    const int n_partials = chunks > 0 ? (int)chunks : 1;
    unsigned* ticket = reinterpret_cast<unsigned*>(ws);
    unsigned long long* partial = reinterpret_cast<unsigned long long*>(reinterpret_cast<char*>(ws) + LOG_TICKET_BYTES);
    const LogOut O = {loss, loss_log, gnorm2_log, acc, first_bad, step};
    int base = 0, t = 0;
    do {                                             // one launch per LOG_MAX_T non-empty tensors (one in all for the models here)
        LogTable T;
        T.count = 0;
        int local = 0;
        long long local_elems = 0;
        for (; t < n_tensors && T.count < LOG_MAX_T; ++t) {
            if (numel[t] == 0) continue;
            const int k = T.count++;
            T.g[k] = grads[t];
            T.n[k] = numel[t];
            T.first_chunk[k] = local;
            local_elems += numel[t];
            local += (int)((numel[t] + LOG_CHUNK - 1) / LOG_CHUNK);
        }
        for (int k = T.count; k < LOG_MAX_T; ++k) { T.g[k] = nullptr; T.n[k] = 0; }
        for (int k = T.count; k <= LOG_MAX_T; ++k) T.first_chunk[k] = local;
        if (T.count == 0 && base > 0) break;         // trailing empty tensors: every partial is already on its way
        // compulsory bytes: this launch's gradients once and its partials' stores; the step's last launch also reads every partial and
        // writes the log row
        const bool final_launch = base + local >= n_partials;
        ProfScope prof("step_log_kernel", (hipStream_t)stream, 4.0 * local_elems + 8.0 * (local > 0 ? local : 1) + (final_launch ? 8.0 * n_partials + 32.0 : 0.0), 1);
        hipLaunchKernelGGL(step_log_kernel, dim3((unsigned)(local > 0 ? local : 1)), dim3(LOG_THREADS), 0, (hipStream_t)stream, T, O, ticket,
                           partial, base, n_partials);
        TXE_CHECK_LAUNCH();
        base += local;
    } while (t < n_tensors);
    return TXE_OK;
}

}  // extern "C"
