// Adam / AMSGrad update of the whole parameter set in ONE launch (trainer.py:61 `self.optimizer.step()` with the optimizer of
// config.mag.json:66-73: Adam, lr 1e-3, weight_decay 0, amsgrad true).
// The model has 9 parameter tensors of very unequal sizes (3 ... 1,025,000 elements, 1.76 M in total); a multi-tensor apply that
// hands 64 K-element chunks to workgroups puts 27 workgroups on 256 CUs.  Here every workgroup owns 1,024 consecutive elements of
// one tensor (1,700 workgroups), 16-byte accesses: 9 streams x 7 MB = HBM-bound.
// The same launch can keep an exponential moving average of the parameters (txe_adam_step_ema: two more streams), and
// tensor_swap_kernel exchanges the parameters with those averages in one launch of the same shape (txe_tensor_swap).
#include "txe_common.h"
#include "txe_adam.h"          // AdamScalars, adam_scalars, adam_one: the update itself, shared with txe_rowgrad.hip

#include <math.h>

namespace txe {

constexpr int ADAM_MAX_T = 24;          // tensors per launch (kernel-argument table)
constexpr int ADAM_CHUNK = 1024;        // elements per workgroup

struct AdamTable {
    float* p[ADAM_MAX_T];
    const float* g[ADAM_MAX_T];
    float* m[ADAM_MAX_T];
    float* v[ADAM_MAX_T];
    float* vmax[ADAM_MAX_T];
    long long n[ADAM_MAX_T];
    int first_chunk[ADAM_MAX_T + 1];
    int count;
};

// The averaged weights of txe_adam_step_ema: a seventh pointer table beside AdamTable's (same order of tensors) and 1 - decay of this step.
// Only the EMA kernels take it; adam_kernel / adam_guarded_kernel have the arguments they had.
struct AdamEma {
    float* e[ADAM_MAX_T];
    float one_minus_d;
};

// The guard of one step (txe_adam_step_guarded): two device scalars that work enqueued EARLIER ON THE SAME STREAM has written (the
// step log's first_bad word and its gnorm2 slot of this step) and the host's clip threshold.  Either pointer may be null.  Both are
// only read -- one wave-uniform load each, once per workgroup, before any per-element work.
struct AdamGuard {
    const long long* first_bad;     // *first_bad >= 0: the whole step is skipped (no load, no store)
    const double* gnorm2;           // the squared global L2 norm of the gradients: every g is scaled by min(1, max_norm / (sqrt(.) + 1e-6))
    double max_grad_norm;
};

// e = lerp(e, p_new, 1 - decay) in the form m has: one subtraction, one fma (optim.host_ema_update restates it); p_new is the fp32 value
// that the same thread stores
__device__ __forceinline__ void ema_one(float& e, float p_new, float one_minus_d) { e = fmaf(one_minus_d, p_new - e, e); }

template <bool AMS, bool GUARD, bool EMA = false>
__device__ __forceinline__ void adam_chunk(const AdamTable& T, const AdamScalars& c, float coef, const AdamEma* ema = nullptr) {
    int t = 0;
#pragma unroll 1
    while (t + 1 < T.count && (int)blockIdx.x >= T.first_chunk[t + 1]) ++t;
    const long long n = T.n[t];
    const long long i0 = (long long)(blockIdx.x - T.first_chunk[t]) * ADAM_CHUNK + 4 * threadIdx.x;
    if (i0 >= n) return;
    float* __restrict__ P = T.p[t];
    const float* __restrict__ G = T.g[t];
    float* __restrict__ M = T.m[t];
    float* __restrict__ V = T.v[t];
    float* __restrict__ X = AMS ? T.vmax[t] : T.v[t];
    float* __restrict__ E = EMA ? ema->e[t] : nullptr;
    const float omd = EMA ? ema->one_minus_d : 0.f;
    const bool vec = (i0 + 3 < n) && ((((uintptr_t)P | (uintptr_t)G | (uintptr_t)M | (uintptr_t)V | (uintptr_t)X | (uintptr_t)E) & 15) == 0);
    if (vec) {
        float4 p = *reinterpret_cast<const float4*>(P + i0);
        const float4 g = *reinterpret_cast<const float4*>(G + i0);
        float4 m = *reinterpret_cast<const float4*>(M + i0);
        float4 v = *reinterpret_cast<const float4*>(V + i0);
        float4 x = *reinterpret_cast<const float4*>(X + i0);
        float4 e;
        if (EMA) e = *reinterpret_cast<const float4*>(E + i0);
        adam_one<GUARD>(p.x, g.x, m.x, v.x, x.x, AMS, c, coef);
        adam_one<GUARD>(p.y, g.y, m.y, v.y, x.y, AMS, c, coef);
        adam_one<GUARD>(p.z, g.z, m.z, v.z, x.z, AMS, c, coef);
        adam_one<GUARD>(p.w, g.w, m.w, v.w, x.w, AMS, c, coef);
        *reinterpret_cast<float4*>(P + i0) = p;
        *reinterpret_cast<float4*>(M + i0) = m;
        *reinterpret_cast<float4*>(V + i0) = v;
        if (AMS) *reinterpret_cast<float4*>(X + i0) = x;
        if (EMA) {
            ema_one(e.x, p.x, omd);
            ema_one(e.y, p.y, omd);
            ema_one(e.z, p.z, omd);
            ema_one(e.w, p.w, omd);
            *reinterpret_cast<float4*>(E + i0) = e;
        }
    } else {
        for (long long i = i0; i < n && i < i0 + 4; ++i) {
            float p = P[i], m = M[i], v = V[i], x = AMS ? X[i] : 0.f;
            adam_one<GUARD>(p, G[i], m, v, x, AMS, c, coef);
            P[i] = p; M[i] = m; V[i] = v;
            if (AMS) X[i] = x;
            if (EMA) {
                float e = E[i];
                ema_one(e, p, omd);
                E[i] = e;
            }
        }
    }
}

template <bool AMS>
__global__ __launch_bounds__(256) void adam_kernel(AdamTable T, AdamScalars c) {
    adam_chunk<AMS, false>(T, c, 1.f);
}

// adam_kernel behind the guard.  The coefficient is clip_grad_norm_'s, formed in fp64: max_norm / (norm + 1e-6), used when below 1.  A
// norm that is not finite, met without a first_bad pointer, goes through the same formula: NaN compares false and leaves the
// coefficient at 1, +Inf gives 0 (and 0 * Inf = NaN in the elements that are Inf) -- no parity with torch is claimed there.
template <bool AMS>
__global__ __launch_bounds__(256) void adam_guarded_kernel(AdamTable T, AdamScalars c, AdamGuard G) {
    if (G.first_bad && G.first_bad[0] >= 0) return;         // frozen: p, m, v and vmax stay as they are
    float coef = 1.f;
    if (G.gnorm2) {
        const double coef64 = G.max_grad_norm / (sqrt(G.gnorm2[0]) + 1e-6);
        coef = coef64 < 1.0 ? (float)coef64 : 1.0f;
    }
    adam_chunk<AMS, true>(T, c, coef);
}

// adam_kernel / adam_guarded_kernel with the average of the parameters formed beside the update: one more 16-byte load and store per
// thread, everything else as above (the guard's early return comes before any load: a frozen step leaves e alone too)
template <bool AMS>
__global__ __launch_bounds__(256) void adam_ema_kernel(AdamTable T, AdamScalars c, AdamEma E) {
    adam_chunk<AMS, false, true>(T, c, 1.f, &E);
}

template <bool AMS>
__global__ __launch_bounds__(256) void adam_guarded_ema_kernel(AdamTable T, AdamScalars c, AdamGuard G, AdamEma E) {
    if (G.first_bad && G.first_bad[0] >= 0) return;         // frozen: p, m, v, vmax and e stay as they are
    float coef = 1.f;
    if (G.gnorm2) {
        const double coef64 = G.max_grad_norm / (sqrt(G.gnorm2[0]) + 1e-6);
        coef = coef64 < 1.0 ? (float)coef64 : 1.0f;
    }
    adam_chunk<AMS, true, true>(T, c, coef, &E);
}

// a[t][i] <-> b[t][i] as 32-bit words (no float ever exists: NaN payloads, -0.0 and denormals pass through), chunked as the Adam kernels
struct SwapTable {
    unsigned* a[ADAM_MAX_T];
    unsigned* b[ADAM_MAX_T];
    long long n[ADAM_MAX_T];
    int first_chunk[ADAM_MAX_T + 1];
    int count;
};

__global__ __launch_bounds__(256) void tensor_swap_kernel(SwapTable T) {
    int t = 0;
#pragma unroll 1
    while (t + 1 < T.count && (int)blockIdx.x >= T.first_chunk[t + 1]) ++t;
    const long long n = T.n[t];
    const long long i0 = (long long)(blockIdx.x - T.first_chunk[t]) * ADAM_CHUNK + 4 * threadIdx.x;
    if (i0 >= n) return;
    unsigned* __restrict__ A = T.a[t];
    unsigned* __restrict__ B = T.b[t];
    if ((i0 + 3 < n) && ((((uintptr_t)A | (uintptr_t)B) & 15) == 0)) {
        const uint4 a = *reinterpret_cast<const uint4*>(A + i0);
        const uint4 b = *reinterpret_cast<const uint4*>(B + i0);
        *reinterpret_cast<uint4*>(A + i0) = b;
        *reinterpret_cast<uint4*>(B + i0) = a;
    } else {
        for (long long i = i0; i < n && i < i0 + 4; ++i) {
            const unsigned a = A[i], b = B[i];
            A[i] = b; B[i] = a;
        }
    }
}

}  // namespace txe

using namespace txe;

namespace {

// txe_adam_step, txe_adam_step_guarded and txe_adam_step_ema; guard == nullptr launches adam_kernel, anything else adam_guarded_kernel
// over the same tables; ema != nullptr launches their EMA variants with the seventh table
int adam_step(int n_tensors, float* const* params, const float* const* grads, float* const* exp_avg, float* const* exp_avg_sq,
              float* const* max_exp_avg_sq, const long long* numel, double lr, double beta1, double beta2, double eps, double weight_decay,
              long long step, const AdamGuard* guard, void* stream, float* const* ema = nullptr, double ema_decay = 0.0) {
    if (n_tensors < 0 || step < 1 || (n_tensors > 0 && (!params || !grads || !exp_avg || !exp_avg_sq || !numel))) return TXE_ERR_ARG;
    if (!(beta1 >= 0.0 && beta1 < 1.0 && beta2 >= 0.0 && beta2 < 1.0)) return TXE_ERR_ARG;
    const AdamScalars c = adam_scalars(lr, beta1, beta2, eps, weight_decay, step);
    const bool ams = max_exp_avg_sq != nullptr;
    AdamEma E;
    E.one_minus_d = (float)(1.0 - ema_decay);
    for (int t = 0; t < n_tensors;) {                  // one launch per ADAM_MAX_T non-empty tensors
        AdamTable T;
        T.count = 0;
        long long chunks = 0, elems = 0;
        for (; t < n_tensors && T.count < ADAM_MAX_T; ++t) {
            if (numel[t] < 0) return TXE_ERR_ARG;
            if (numel[t] == 0) continue;
            if (!params[t] || !grads[t] || !exp_avg[t] || !exp_avg_sq[t] || (ams && !max_exp_avg_sq[t]) || (ema && !ema[t])) return TXE_ERR_ARG;
            const int k = T.count++;
            E.e[k] = ema ? ema[t] : nullptr;
            T.p[k] = params[t]; T.g[k] = grads[t]; T.m[k] = exp_avg[t]; T.v[k] = exp_avg_sq[t];
            T.vmax[k] = ams ? max_exp_avg_sq[t] : exp_avg_sq[t];
            T.n[k] = numel[t];
            elems += numel[t];
            T.first_chunk[k] = (int)chunks;
            chunks += (numel[t] + ADAM_CHUNK - 1) / ADAM_CHUNK;
            if (chunks > 0x7fffffffLL) return TXE_ERR_ARG;
        }
        if (T.count == 0) continue;
        T.first_chunk[T.count] = (int)chunks;
        for (int k = T.count; k < ADAM_MAX_T; ++k) { T.p[k] = nullptr; T.g[k] = nullptr; T.m[k] = nullptr; T.v[k] = nullptr; T.vmax[k] = nullptr; T.n[k] = 0; T.first_chunk[k + 1] = (int)chunks; E.e[k] = nullptr; }
        const double bytes = 4.0 * elems * (ams ? 9 : 7);          // p, g, m, v [, vmax] read; all but g written (a frozen step moves none of it)
        if (ema) {                                                 // e read and written: 8 more bytes per element
            if (guard) {
                ProfScope prof(ams ? "adam_guarded_ema_kernel<true>" : "adam_guarded_ema_kernel<false>", (hipStream_t)stream, bytes + 8.0 * elems + 16.0, 1);
                if (ams) hipLaunchKernelGGL(adam_guarded_ema_kernel<true>, dim3((unsigned)chunks), dim3(256), 0, (hipStream_t)stream, T, c, *guard, E);
                else hipLaunchKernelGGL(adam_guarded_ema_kernel<false>, dim3((unsigned)chunks), dim3(256), 0, (hipStream_t)stream, T, c, *guard, E);
                TXE_CHECK_LAUNCH();
            } else {
                ProfScope prof(ams ? "adam_ema_kernel<true>" : "adam_ema_kernel<false>", (hipStream_t)stream, bytes + 8.0 * elems, 1);
                if (ams) hipLaunchKernelGGL(adam_ema_kernel<true>, dim3((unsigned)chunks), dim3(256), 0, (hipStream_t)stream, T, c, E);
                else hipLaunchKernelGGL(adam_ema_kernel<false>, dim3((unsigned)chunks), dim3(256), 0, (hipStream_t)stream, T, c, E);
                TXE_CHECK_LAUNCH();
            }
        } else if (guard) {
            ProfScope prof(ams ? "adam_guarded_kernel<true>" : "adam_guarded_kernel<false>", (hipStream_t)stream, bytes + 16.0, 1);
            if (ams) hipLaunchKernelGGL(adam_guarded_kernel<true>, dim3((unsigned)chunks), dim3(256), 0, (hipStream_t)stream, T, c, *guard);
            else hipLaunchKernelGGL(adam_guarded_kernel<false>, dim3((unsigned)chunks), dim3(256), 0, (hipStream_t)stream, T, c, *guard);
            TXE_CHECK_LAUNCH();
        } else {
            ProfScope prof(ams ? "adam_kernel<true>" : "adam_kernel<false>", (hipStream_t)stream, bytes, 1);
            if (ams) hipLaunchKernelGGL(adam_kernel<true>, dim3((unsigned)chunks), dim3(256), 0, (hipStream_t)stream, T, c);
            else hipLaunchKernelGGL(adam_kernel<false>, dim3((unsigned)chunks), dim3(256), 0, (hipStream_t)stream, T, c);
            TXE_CHECK_LAUNCH();
        }
    }
    return TXE_OK;
}

}  // namespace

extern "C" {

// One optimizer step over n_tensors parameter tensors (HOST arrays of DEVICE pointers; numel[t] elements each, fp32, dense).
//   g' = g + weight_decay p;  m = lerp(m, g', 1-beta1);  v = beta2 v + (1-beta2) g'^2;  [vmax = max(vmax, v)]
//   p -= lr / (1 - beta1^step) * m / (sqrt(vmax or v) / sqrt(1 - beta2^step) + eps)
// `step` is the 1-based count of THIS update (shared by the tensors of the call); max_exp_avg_sq == NULL selects plain Adam.
int txe_adam_step(int n_tensors, float* const* params, const float* const* grads, float* const* exp_avg, float* const* exp_avg_sq,
                  float* const* max_exp_avg_sq, const long long* numel, double lr, double beta1, double beta2, double eps,
                  double weight_decay, long long step, void* stream) {
    return adam_step(n_tensors, params, grads, exp_avg, exp_avg_sq, max_exp_avg_sq, numel, lr, beta1, beta2, eps, weight_decay, step, nullptr,
                     stream);
}

// txe_adam_step behind two DEVICE scalars written by earlier work on the same stream (include/txe.h): *first_bad >= 0 skips the step,
// g is scaled by min(1, max_grad_norm / (sqrt(*gnorm2) + 1e-6)).  Both NULL: txe_adam_step itself, the same launches.
int txe_adam_step_guarded(int n_tensors, float* const* params, const float* const* grads, float* const* exp_avg, float* const* exp_avg_sq,
                          float* const* max_exp_avg_sq, const long long* numel, double lr, double beta1, double beta2, double eps,
                          double weight_decay, long long step, const double* gnorm2, const long long* first_bad, double max_grad_norm,
                          void* stream) {
    if (gnorm2 && !(isfinite(max_grad_norm) && max_grad_norm > 0.0)) return TXE_ERR_ARG;
    const AdamGuard guard = {first_bad, gnorm2, gnorm2 ? max_grad_norm : 0.0};
    return adam_step(n_tensors, params, grads, exp_avg, exp_avg_sq, max_exp_avg_sq, numel, lr, beta1, beta2, eps, weight_decay, step,
                     (gnorm2 || first_bad) ? &guard : nullptr, stream);
}

// txe_adam_step_guarded with the exponential moving average of the parameters formed in the same launches (include/txe.h):
//   e = fma(1 - ema_decay, p_new - e, e), p_new the fp32 parameter this step stores; a frozen step leaves e alone.
// ema == NULL: txe_adam_step_guarded itself (ema_decay is not looked at).
int txe_adam_step_ema(int n_tensors, float* const* params, const float* const* grads, float* const* exp_avg, float* const* exp_avg_sq,
                      float* const* max_exp_avg_sq, float* const* ema, const long long* numel, double lr, double beta1, double beta2,
                      double eps, double weight_decay, long long step, double ema_decay, const double* gnorm2, const long long* first_bad,
                      double max_grad_norm, void* stream) {
    if (ema && !(ema_decay >= 0.0 && ema_decay < 1.0)) return TXE_ERR_ARG;         // first: checkable with no tensor and no device
    if (!ema)
        return txe_adam_step_guarded(n_tensors, params, grads, exp_avg, exp_avg_sq, max_exp_avg_sq, numel, lr, beta1, beta2, eps, weight_decay,
                                     step, gnorm2, first_bad, max_grad_norm, stream);
    if (gnorm2 && !(isfinite(max_grad_norm) && max_grad_norm > 0.0)) return TXE_ERR_ARG;
    const AdamGuard guard = {first_bad, gnorm2, gnorm2 ? max_grad_norm : 0.0};
    return adam_step(n_tensors, params, grads, exp_avg, exp_avg_sq, max_exp_avg_sq, numel, lr, beta1, beta2, eps, weight_decay, step,
                     (gnorm2 || first_bad) ? &guard : nullptr, stream, ema, ema_decay);
}

// a[t] <-> b[t], bit for bit, n_tensors pairs of numel[t] 32-bit words (HOST arrays of DEVICE pointers), ADAM_MAX_T pairs per launch.
// The two tensors of a pair, and different pairs, must not overlap.
int txe_tensor_swap(int n_tensors, float* const* a, float* const* b, const long long* numel, void* stream) {
    if (n_tensors < 0 || (n_tensors > 0 && (!a || !b || !numel))) return TXE_ERR_ARG;
    for (int t = 0; t < n_tensors; ++t)                 // every pair is checked before the first launch
        if (numel[t] < 0 || (numel[t] > 0 && (!a[t] || !b[t]))) return TXE_ERR_ARG;
    for (int t = 0; t < n_tensors;) {
        SwapTable T;
        T.count = 0;
        long long chunks = 0, elems = 0;
        for (; t < n_tensors && T.count < ADAM_MAX_T; ++t) {
            if (numel[t] == 0) continue;
            const int k = T.count++;
            T.a[k] = reinterpret_cast<unsigned*>(a[t]); T.b[k] = reinterpret_cast<unsigned*>(b[t]);
            T.n[k] = numel[t];
            elems += numel[t];
            T.first_chunk[k] = (int)chunks;
            chunks += (numel[t] + ADAM_CHUNK - 1) / ADAM_CHUNK;
            if (chunks > 0x7fffffffLL) return TXE_ERR_ARG;
        }
        if (T.count == 0) continue;
        T.first_chunk[T.count] = (int)chunks;
        for (int k = T.count; k < ADAM_MAX_T; ++k) { T.a[k] = nullptr; T.b[k] = nullptr; T.n[k] = 0; T.first_chunk[k + 1] = (int)chunks; }
        ProfScope prof("tensor_swap_kernel", (hipStream_t)stream, 16.0 * elems, 1);      // both tensors read and written
        hipLaunchKernelGGL(tensor_swap_kernel, dim3((unsigned)chunks), dim3(256), 0, (hipStream_t)stream, T);
        TXE_CHECK_LAUNCH();
    }
    return TXE_OK;
}

}  // extern "C"
