// Fused softmax-cross-entropy over a large vocabulary for gfx950.
//
// GPT-2's loss is cross_entropy over [R = B*T, V ~ 50k] bf16 logits; the
// torch path (log_softmax fwd + bwd + nll kernels) reads/writes the logit
// matrix several times in fp32 (~6% of the training step). Here:
//
//   fwd: one ONLINE max+sum pass per row (single global read of the
//        logits, short8-vectorized), block reduction merging (m, s)
//        pairs, saves per-row lse for backward and the mean loss via a
//        two-stage deterministic reduction on the host side.
//   bwd: dlogits = (softmax - onehot) * scale in one elementwise pass
//        (one read + one write).
//
// Numerics: accumulation fp32, exp via __expf. Per-row lse and loss stay
// within 16x the deviation of fp32 torch.logsumexp from fp64, dlogits within
// one bf16 rounding of the fp64 gradient
// (tests/test_gpu_kernel_edges.py, docs/KERNELS.md).

#include <torch/extension.h>
#include <c10/hip/HIPStream.h>
#include <hip/hip_bf16.h>

#include "ops_common.h"

namespace dmlamd {

typedef short short8 __attribute__((ext_vector_type(8)));

__device__ __forceinline__ float bf2f_(unsigned short b) {
  __hip_bfloat16 h;
  __builtin_memcpy(&h, &b, 2);
  return __bfloat162float(h);
}

// Merge two online-softmax (max, sum) pairs.
__device__ __forceinline__ void online_merge(float& m, float& s, float m2, float s2) {
  const float mn = fmaxf(m, m2);
  s = s * __expf(m - mn) + s2 * __expf(m2 - mn);
  m = mn;
}

// One block per row; per-row loss and lse. Rows whose target equals
// ignore_index contribute loss 0 (the host wrapper divides by the valid
// count — F.cross_entropy ignore_index semantics). A target outside
// [0, V) that is NOT ignore_index writes NaN instead of reading out of
// bounds: loud, not garbage.
__global__ void __launch_bounds__(kBlock) ce_fwd_kernel(
    const __hip_bfloat16* __restrict__ logits, const int64_t* __restrict__ targets,
    float* __restrict__ loss_out, float* __restrict__ lse_out, int64_t R, int64_t V,
    int64_t ignore_index) {
  __shared__ float lds_m[kBlock / kWave];
  __shared__ float lds_s[kBlock / kWave];

  const int lane = threadIdx.x & (kWave - 1);
  const int wave = threadIdx.x / kWave;
  const int64_t nvec = V / 8;

  for (int64_t row = blockIdx.x; row < R; row += gridDim.x) {
    const short8* lr = (const short8*)(logits + row * V);
    float m = -1e30f, s = 0.0f;
    for (int64_t i = threadIdx.x; i < nvec; i += kBlock) {
      unsigned short v[8];
      *(short8*)v = lr[i];
      float cm = -1e30f;
#pragma unroll
      for (int k = 0; k < 8; ++k) cm = fmaxf(cm, bf2f_(v[k]));
      float cs = 0.0f;
#pragma unroll
      for (int k = 0; k < 8; ++k) cs += __expf(bf2f_(v[k]) - cm);
      online_merge(m, s, cm, cs);
    }
    for (int64_t i = nvec * 8 + threadIdx.x; i < V; i += kBlock) {
      // __bfloat162float, not bf2f_: passing a __hip_bfloat16 where bf2f_
      // takes raw bits converts its VALUE to an integer first
      online_merge(m, s, __bfloat162float(logits[row * V + i]), 1.0f);
    }
    // wave merge
#pragma unroll
    for (int off = kWave / 2; off > 0; off >>= 1) {
      const float m2 = __shfl_down(m, off, kWave);
      const float s2 = __shfl_down(s, off, kWave);
      online_merge(m, s, m2, s2);
    }
    if (lane == 0) {
      lds_m[wave] = m;
      lds_s[wave] = s;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
      float mt = lds_m[0], st = lds_s[0];
#pragma unroll
      for (int w = 1; w < kBlock / kWave; ++w) online_merge(mt, st, lds_m[w], lds_s[w]);
      const float lse = mt + __logf(st);
      lse_out[row] = lse;
      const int64_t tgt = targets[row];
      if (tgt == ignore_index) {
        loss_out[row] = 0.0f;
      } else if (tgt < 0 || tgt >= V) {
        loss_out[row] = __builtin_nanf("");
      } else {
        const float xt = __bfloat162float(((const __hip_bfloat16*)logits)[row * V + tgt]);
        loss_out[row] = lse - xt;
      }
    }
    __syncthreads();
  }
}

// dlogits = (exp(x - lse) - onehot) * scale  (scale folds the mean + any
// upstream grad; elementwise over R x V). Ignored / out-of-range rows
// write zero gradients.
__global__ void __launch_bounds__(kBlock) ce_bwd_kernel(
    const __hip_bfloat16* __restrict__ logits, const int64_t* __restrict__ targets,
    const float* __restrict__ lse_in, const float* __restrict__ scale_ptr,
    __hip_bfloat16* __restrict__ dlogits, int64_t R, int64_t V, int64_t ignore_index) {
  const float scale = scale_ptr[0];
  const int64_t nvec = V / 8;
  const int64_t stride = (int64_t)gridDim.x * kBlock;
  const __hip_bfloat16 zero_bf = __float2bfloat16(0.0f);

  for (int64_t t = (int64_t)blockIdx.x * kBlock + threadIdx.x; t < R * nvec; t += stride) {
    const int64_t row = t / nvec;
    const int64_t i = t - row * nvec;
    const float lse = lse_in[row];
    const int64_t tgt = targets[row];
    const bool valid = tgt >= 0 && tgt < V && tgt != ignore_index;
    unsigned short v[8], o[8];
    *(short8*)v = ((const short8*)(logits + row * V))[i];
#pragma unroll
    for (int k = 0; k < 8; ++k) {
      const int64_t col = i * 8 + k;
      float p = __expf(bf2f_(v[k]) - lse);
      if (col == tgt) p -= 1.0f;
      const __hip_bfloat16 h = valid ? __float2bfloat16(p * scale) : zero_bf;
      __builtin_memcpy(&o[k], &h, 2);
    }
    ((short8*)(dlogits + row * V))[i] = *(short8*)o;
  }
  // scalar tail columns
  for (int64_t t = (int64_t)blockIdx.x * kBlock + threadIdx.x; t < R * (V - nvec * 8);
       t += stride) {
    const int64_t row = t / (V - nvec * 8);
    const int64_t col = nvec * 8 + (t - row * (V - nvec * 8));
    const int64_t tgt = targets[row];
    const bool valid = tgt >= 0 && tgt < V && tgt != ignore_index;
    float p = __expf(__bfloat162float(((const __hip_bfloat16*)logits)[row * V + col]) -
                     lse_in[row]);
    if (col == tgt) p -= 1.0f;
    ((__hip_bfloat16*)dlogits)[row * V + col] = valid ? __float2bfloat16(p * scale) : zero_bf;
  }
}

void ce_fwd(at::Tensor logits, at::Tensor targets, at::Tensor loss, at::Tensor lse,
            int64_t ignore_index) {
  TORCH_CHECK(logits.is_cuda() && logits.scalar_type() == at::kBFloat16 && logits.is_contiguous(),
              "logits must be contiguous bf16");
  TORCH_CHECK(targets.scalar_type() == at::kLong, "targets must be int64");
  const int64_t V = logits.size(-1);
  const int64_t R = logits.numel() / V;
  TORCH_CHECK(targets.numel() == R, "targets must have one entry per logit row");
  TORCH_CHECK(loss.scalar_type() == at::kFloat && loss.numel() >= R, "loss must be fp32[R]");
  TORCH_CHECK(lse.scalar_type() == at::kFloat && lse.numel() >= R, "lse must be fp32[R]");
  auto stream = c10::hip::getCurrentHIPStream();
  const int blocks = (int)std::min<int64_t>(R, kMaxGrid);
  hipLaunchKernelGGL(ce_fwd_kernel, dim3(blocks), dim3(kBlock), 0, stream,
                     (const __hip_bfloat16*)logits.data_ptr(), targets.data_ptr<int64_t>(),
                     loss.data_ptr<float>(), lse.data_ptr<float>(), R, V, ignore_index);
}

void ce_bwd(at::Tensor logits, at::Tensor targets, at::Tensor lse, at::Tensor scale,
            at::Tensor dlogits, int64_t ignore_index) {
  const int64_t V = logits.size(-1);
  const int64_t R = logits.numel() / V;
  TORCH_CHECK(targets.numel() == R, "targets must have one entry per logit row");
  TORCH_CHECK(dlogits.sizes() == logits.sizes() && dlogits.scalar_type() == at::kBFloat16,
              "dlogits must match logits");
  auto stream = c10::hip::getCurrentHIPStream();
  const int blocks = grid_for(R * (V / 8), kBlock);
  hipLaunchKernelGGL(ce_bwd_kernel, dim3(blocks), dim3(kBlock), 0, stream,
                     (const __hip_bfloat16*)logits.data_ptr(), targets.data_ptr<int64_t>(),
                     lse.data_ptr<float>(), scale.data_ptr<float>(),
                     (__hip_bfloat16*)dlogits.data_ptr(), R, V, ignore_index);
}

} // namespace dmlamd
