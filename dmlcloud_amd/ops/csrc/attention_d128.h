// Head dim 128 forms of the flash-attention kernels. Part of attention.hip
// (included at its end, inside namespace dmlamd): the fragment maps, vt_idx
// images, crow / dstart / bwd_prob and the kRagged / kDoc / kGqa flags are the
// ones documented there, and every clamping, masking, skipping and diagonal
// argument that stands next to a loop of the D = 64 kernels holds for the loop
// of the same name here: none of them depends on D. What differs is how a
// 128-wide row moves through LDS and registers:
//   * a [rows][128] tile that is read transposed (V in the forward, Q and dO
//     in dK/dV, K in dQ) is TWO vt_idx images per 32 rows, D columns 0..63 and
//     64..127, selected by col / 64; read_tr_frag is used as it is;
//   * a row-major K/V tile has row stride kKVStrideD128 = 136 bf16 = 68
//     dwords, gcd(68, 64) = 4: the 16 rows one b128 fragment read touches at
//     one column offset start in 16 distinct bank groups, as with stride 88;
//   * S^T = K Q^T and dP^T = V dO^T contract over four 32-wide chunks, the
//     PV / dV / dK / dQ products write eight 16-wide D chunks.
// The code is compiled without packed-fp32 instructions (kD128Fn), like the
// decode kernels, and uses their decode_shfl / decode_barrier.
#pragma once

#define kD128Fn __attribute__((target("no-packed-fp32-ops")))

constexpr int kKVStrideD128 = 136;
constexpr int kDChunks128 = kAttnD128 / 16; // 16-wide output chunks
constexpr int kKChunks128 = kAttnD128 / 32; // 32-wide contraction chunks

// ---------------------------------------------------------------- forward
// Block = 4 waves on consecutive q rows of one (b, h); 64-key K/V tiles
// stream past through the write-late double buffer of the D = 64 kernel. A
// 64x128 tile is 1024 bf16x8 pieces, four per thread: rows st_row + 16x,
// columns st_col..+7, a 256-byte row per 16 threads.
// Register budget: the D = 64 kernel holds 204 VGPRs + 32 AGPRs at 2
// waves/SIMD (256 registers per lane). Doubling D in place (qf 32, o_acc 64,
// vf 64, prefetch 32, scores 16, ...) needs about 330. Two forms fit, both
// this one template:
//   kSubs = 2: a wave owns two 16-row sub-tiles (128-row block). Per key
//     tile it first computes S, the softmax and P for BOTH sub-tiles (the P
//     slice in LDS is reused, each sub-tile's two A fragments of P wait in 8
//     registers), then walks P V in two 64-wide D halves, so only one half's
//     8 V fragments (32 registers) are live and still feed both sub-tiles.
//   kSubs = 1: a wave owns one sub-tile (64-row block); half the q-side
//     registers, but every K and V fragment read from LDS feeds half the MFMAs.
// LDS is the same for both: K 2 x 64 x 136 x 2 B = 34816, V 2 x 4 images =
// 32768, P 4 x 16 x 72 x 2 B = 9216, 76800 B in all: two blocks per CU, which
// is also what 2 waves/SIMD asks for. The compiler's verdict
// (profiles/attention_d128.txt): kSubs = 2 takes 244..256 VGPRs + 72..96
// AGPRs, ONE wave/SIMD; forced to two with amdgpu_waves_per_eu(2, 2) the
// dense instantiations spill 20 VGPRs (84 B/lane) in the key loop. kSubs = 1
// takes 173..216 VGPRs + 40 AGPRs, two waves/SIMD, no spill, and is what the
// launcher runs (kFwdSubsD128). Measured with kSubs = 1 on an MI355X, causal,
// B=8 H=16: 166 us at N=1024 (torch SDPA 164), 605 us at N=2048 (torch 431).
// kSubs = 2 at one wave/SIMD has NOT been measured.
template <int kSubs, bool kRagged, bool kDoc, bool kGqa>
kD128Fn __global__ void __launch_bounds__(kAttnThreads) attn_fwd_d128_kernel(
    const __hip_bfloat16* __restrict__ q, const __hip_bfloat16* __restrict__ k,
    const __hip_bfloat16* __restrict__ v, __hip_bfloat16* __restrict__ o,
    float* __restrict__ lse, int BH, int H, int N, float scale, bool causal_arg, Strides sq,
    StridesGqa<kGqa> sk, StridesDoc<kDoc> sv) {
  const bool causal = kDoc || causal_arg; // a document mask is causal by contract
  constexpr int kRows = kWavesPerBlock * kSubs * kQT; // q rows per block
  __shared__ __hip_bfloat16 p_lds_all[kWavesPerBlock][kQT][kPStrideF];
  __shared__ __hip_bfloat16 k_lds[2][kKTF][kKVStrideD128];
  // image (2c + dh) of a buffer: keys 32c..32c+31, D columns 64dh..64dh+63
  __shared__ __hip_bfloat16 v_tr[2][4 * kImgElems];

  const Coords tc = thread_coords();
  const int lane = tc.lane, wave = tc.wave, row16 = tc.row16, grp = tc.grp;
  const int st_row = threadIdx.x >> 4; // 0..15; pieces at rows st_row + 16x
  const int st_col = (threadIdx.x & 15) * 8; // 0..120
  __hip_bfloat16(*p_lds)[kPStrideF] = p_lds_all[wave];
  // piece x of V sits in image 2(x / 2) + st_col / 64; inside an image 16
  // rows further down is 128 elements further on (vt_idx: row / 8 counts 64s)
  const int st_vt = (st_col >> 6) * kImgElems + vt_idx(st_row, st_col & 63);
  auto v_off = [&](int x) kD128Fn __attribute__((always_inline)) {
    return (x >> 1) * 2 * kImgElems + (x & 1) * 128 + st_vt;
  };

  const int nqb = (N + kRows - 1) / kRows;
  const int64_t total_blocks = (int64_t)BH * nqb;

  for (int64_t blk = blockIdx.x; blk < total_blocks; blk += gridDim.x) {
    const int bh = blk / nqb;
    const int qb0 = (blk - (int64_t)bh * nqb) * kRows;
    const int i0 = qb0 + wave * kSubs * kQT; // this wave's q rows
    const bool valid = i0 < N;
    const __hip_bfloat16* qp = tslice(q, sq, bh, H);
    const __hip_bfloat16* kp = kv_slice(k, sk, bh, H, sk);
    const __hip_bfloat16* vp = kv_slice(v, sv, bh, H, sk);

    bf16x8 qf[kSubs][kKChunks128]; // [sub-tile][k-chunk]
    if (valid) {
#pragma unroll
      for (int sub = 0; sub < kSubs; ++sub) {
#pragma unroll
        for (int c = 0; c < kKChunks128; ++c) {
          qf[sub][c] =
              *(const bf16x8*)(qp + (int64_t)crow<kRagged>(i0 + 16 * sub + row16, N) * sq.r +
                               32 * c + 8 * grp);
        }
      }
    }

    const float scale2 = scale * kLog2e; // fold log2(e): exp -> v_exp_f32
    float m_run[kSubs], s_run[kSubs];
    f32x4 o_acc[kSubs][kDChunks128];
#pragma unroll
    for (int sub = 0; sub < kSubs; ++sub) {
      m_run[sub] = -1e30f;
      s_run[sub] = 0.0f;
#pragma unroll
      for (int db = 0; db < kDChunks128; ++db) o_acc[sub][db] = f32x4{0, 0, 0, 0};
    }

    // The walk of the D = 64 forward with kRows for its 128: a stored row q
    // of this wave has its diagonal key in the tile j0 = 64 * (q / 64) <= q,
    // q < min(qb0 + kRows, N) = kv_end_block puts that tile below ntiles and
    // j0 <= q < i0 + 16 kSubs = my_kv_end keeps it from being skipped.
    const int kv_end_block = causal ? min(qb0 + kRows, N) : N;
    const int my_kv_end = causal ? (i0 + kSubs * kQT) : N;

    // Documents: the block skip (jt_begin), the sub-tile skip (sub_start)
    // and the wipe, exactly as in the D = 64 forward.
    int jt_begin = 0;
    int q_start[kSubs];
    unsigned q_span[kSubs]; // min(q, N - 1) - start[q] >= 0
    int sub_start[kSubs];
#pragma unroll
    for (int sub = 0; sub < kSubs; ++sub) {
      q_start[sub] = 0;
      q_span[sub] = 0;
      sub_start[sub] = 0;
    }
    if constexpr (kDoc) {
      const int* dsp = sv.doc_start + (int64_t)(bh / H) * N;
      jt_begin = dstart(dsp, qb0, N) / kKTF;
#pragma unroll
      for (int sub = 0; sub < kSubs; ++sub) {
        q_start[sub] = dstart(dsp, i0 + 16 * sub + row16, N);
        q_span[sub] = (unsigned)(min(i0 + 16 * sub + row16, N - 1) - q_start[sub]);
        sub_start[sub] = __builtin_amdgcn_readfirstlane(dstart(dsp, i0 + 16 * sub, N));
      }
    }
    const int j_begin = jt_begin * kKTF;
    const int buf0 = jt_begin & 1;

#pragma unroll
    for (int x = 0; x < 4; ++x) {
      const int64_t row = crow<kRagged>(j_begin + st_row + 16 * x, N);
      *(bf16x8*)(&k_lds[buf0][st_row + 16 * x][st_col]) = *(const bf16x8*)(kp + row * sk.r + st_col);
      *(bf16x8*)(&v_tr[buf0][v_off(x)]) = *(const bf16x8*)(vp + row * sv.r + st_col);
    }
    decode_barrier();

    const int ntiles = (kv_end_block + kKTF - 1) / kKTF;
    for (int jt = jt_begin; jt < ntiles; ++jt) {
      const int j0 = jt * kKTF;
      const int buf = jt & 1;
      bf16x8 knext[4], vnext[4];
      const bool has_next = jt + 1 < ntiles;
      if (has_next) {
#pragma unroll
        for (int x = 0; x < 4; ++x) {
          const int64_t row = crow<kRagged>(j0 + kKTF + st_row + 16 * x, N);
          knext[x] = *(const bf16x8*)(kp + row * sk.r + st_col);
          vnext[x] = *(const bf16x8*)(vp + row * sv.r + st_col);
        }
      }

      if (valid && j0 < my_kv_end) {
        bool act[kSubs]; // wave-uniform: the sub-tile has keys in this tile
        float a_o[kSubs][4]; // the rescale of the O rows this lane holds
        bf16x8 pf[kSubs][2]; // P as the A operand, keys 0..31 and 32..63
#pragma unroll
        for (int sub = 0; sub < kSubs; ++sub) {
          const int qi0 = i0 + 16 * sub;
          act[sub] = !(causal && j0 >= qi0 + kQT); // tile fully past diagonal
          if constexpr (kDoc) {
            if (j0 + kKTF <= sub_start[sub]) act[sub] = false; // wholly in earlier documents
          }
          if (!act[sub]) continue;

          // ---- S^T = K Q^T for four 16-key quarters ----
          float sc[16]; // h*4 + r: key = j0 + 16h + 4grp + r, query = row16
#pragma unroll
          for (int h = 0; h < 4; ++h) {
            f32x4 acc = {0, 0, 0, 0};
#pragma unroll
            for (int c = 0; c < kKChunks128; ++c) {
              const bf16x8 kf = *(const bf16x8*)(&k_lds[buf][16 * h + row16][32 * c + 8 * grp]);
              acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(kf, qf[sub][c], acc, 0, 0, 0);
            }
#pragma unroll
            for (int r = 0; r < 4; ++r) {
              float s = acc[r] * scale2; // log2-domain scores
              const int key_g = j0 + 16 * h + 4 * grp + r;
              if constexpr (kDoc) {
                // start[q] <= key <= min(q, N - 1): document, causal, ragged
                if ((unsigned)(key_g - q_start[sub]) > q_span[sub]) s = -1e30f;
              } else {
                if (causal && key_g > qi0 + row16) s = -1e30f;
                if constexpr (kRagged) {
                  if (key_g >= N) s = -1e30f; // clamped duplicate key
                }
              }
              sc[h * 4 + r] = s;
            }
          }

          // ---- online softmax (per q = row16; reduce across grp groups) ----
          float mt = sc[0];
#pragma unroll
          for (int x = 1; x < 16; ++x) mt = fmaxf(mt, sc[x]);
          mt = fmaxf(mt, decode_shfl(mt, lane ^ 16));
          mt = fmaxf(mt, decode_shfl(mt, lane ^ 32));
          const float m_new = fmaxf(m_run[sub], mt);
          const float alpha = __builtin_amdgcn_exp2f(m_run[sub] - m_new); // -1e30 -> 0
          float ps = 0.0f;
#pragma unroll
          for (int x = 0; x < 16; ++x) {
            sc[x] = __builtin_amdgcn_exp2f(sc[x] - m_new);
            ps += sc[x];
          }
          ps += decode_shfl(ps, lane ^ 16);
          ps += decode_shfl(ps, lane ^ 32);
          s_run[sub] = s_run[sub] * alpha + ps;
          m_run[sub] = m_new;

          // ---- P^T -> the wave's LDS slice, back as two A fragments ----
          // (the next sub-tile reuses the slice: same wave, LDS in order)
#pragma unroll
          for (int h = 0; h < 4; ++h) {
            bf16x4 pw;
#pragma unroll
            for (int r = 0; r < 4; ++r) pw[r] = (__bf16)sc[h * 4 + r];
            *(bf16x4*)(&p_lds[row16][16 * h + 4 * grp]) = pw;
          }
#pragma unroll
          for (int r = 0; r < 4; ++r) a_o[sub][r] = decode_shfl(alpha, 4 * grp + r);
          pf[sub][0] = *(const bf16x8*)(&p_lds[row16][8 * grp]);
          pf[sub][1] = *(const bf16x8*)(&p_lds[row16][32 + 8 * grp]);
        }

        // ---- O = alpha O + P V, one 64-wide D half at a time ----
#pragma unroll
        for (int dh = 0; dh < 2; ++dh) {
          bf16x8 vf[2][4]; // [key chunk][D chunk of the half], shared by the sub-tiles
#pragma unroll
          for (int c = 0; c < 2; ++c) {
#pragma unroll
            for (int db = 0; db < 4; ++db) {
              vf[c][db] = read_tr_frag(&v_tr[buf][(2 * c + dh) * kImgElems], db, lane);
            }
          }
#pragma unroll
          for (int sub = 0; sub < kSubs; ++sub) {
            if (!act[sub]) continue;
#pragma unroll
            for (int db = 0; db < 4; ++db) {
              f32x4& oa = o_acc[sub][4 * dh + db];
#pragma unroll
              for (int r = 0; r < 4; ++r) oa[r] *= a_o[sub][r];
              oa = __builtin_amdgcn_mfma_f32_16x16x32_bf16(pf[sub][0], vf[0][db], oa, 0, 0, 0);
              oa = __builtin_amdgcn_mfma_f32_16x16x32_bf16(pf[sub][1], vf[1][db], oa, 0, 0, 0);
            }
          }
        }
      }
      if (has_next) {
#pragma unroll
        for (int x = 0; x < 4; ++x) {
          *(bf16x8*)(&k_lds[buf ^ 1][st_row + 16 * x][st_col]) = knext[x];
          *(bf16x8*)(&v_tr[buf ^ 1][v_off(x)]) = vnext[x];
        }
      }
      decode_barrier(); // readers of buf done AND buf^1 writes visible
    }

    if (valid) {
      // ---- epilogue: O /= sumexp, store; lse = m + log(sumexp) ----
#pragma unroll
      for (int sub = 0; sub < kSubs; ++sub) {
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int q_o = 4 * grp + r;
          const float denom = decode_shfl(s_run[sub], q_o);
          if (kRagged && i0 + 16 * sub + q_o >= N) continue;
          __bf16* orow = (__bf16*)o + ((int64_t)bh * N + i0 + 16 * sub + q_o) * kAttnD128;
#pragma unroll
          for (int db = 0; db < kDChunks128; ++db) {
            orow[16 * db + row16] = (__bf16)(o_acc[sub][db][r] / denom);
          }
        }
        if (lane < 16 && (!kRagged || i0 + 16 * sub + row16 < N)) {
          // convert the log2-domain stats back to natural-log lse
          lse[(int64_t)bh * N + i0 + 16 * sub + row16] = kLn2 * m_run[sub] + __logf(s_run[sub]);
        }
      }
    }
  }
}

// -------------------------------------------------- delta = rowsum(dO*O)
// One row per 16 lanes, 8 elements per lane; any N, as the D = 64 kernel.
kD128Fn __global__ void __launch_bounds__(kBlock) attn_bwd_delta_d128_kernel(
    const __hip_bfloat16* __restrict__ dout, const __hip_bfloat16* __restrict__ o,
    float* __restrict__ delta, int64_t rows, int H, int N, Strides sdo) {
  const int lane = threadIdx.x & (kWave - 1);
  const int chunk = threadIdx.x & 15;
  const int64_t stride = ((int64_t)gridDim.x * kBlock) / 16;
  for (int64_t r0 = ((int64_t)blockIdx.x * kBlock + threadIdx.x) / 16; r0 < rows; r0 += stride) {
    const int bh = r0 / N;
    const int rr = r0 - (int64_t)bh * N;
    const bf16x8 a = *(const bf16x8*)(tslice(dout, sdo, bh, H) + (int64_t)rr * sdo.r + 8 * chunk);
    const bf16x8 b = *(const bf16x8*)(o + r0 * kAttnD128 + 8 * chunk);
    float s = 0.0f;
#pragma unroll
    for (int j = 0; j < 8; ++j) s += (float)a[j] * (float)b[j];
    // the row's 16 lanes leave the loop together, so every partner is live
#pragma unroll
    for (int off = 8; off > 0; off >>= 1) s += decode_shfl(s, lane ^ off);
    if (chunk == 0) delta[r0] = s;
  }
}

// ------------------------------------------------------------- dK and dV
// The D = 64 kernel's split: a wave owns 16 keys, the block 64, and 32-row
// Q / dO steps stream past as two images each (1024 pieces, two per thread
// and tensor: columns st_col and 64 + st_col of row st_row). Per step and
// wave: 8 MFMAs S^T, 8 dP^T, 8 + 8 into the 64 accumulator registers. A
// group's G heads add into the same accumulators; one rounding, one store.
// ONE block per (b, K/V head, key block), no grid-stride loop: the launcher's
// grid is the exact block count. With the loop, everything the next
// iteration needs (k, v, their strides) stays live in SGPRs through the
// q-step loop, and <kDoc, kGqa> spilled 3 to 9 SGPRs at the limit of 106.
template <bool kRagged, bool kDoc, bool kGqa>
kD128Fn __global__ void __launch_bounds__(kAttnThreads) attn_bwd_dkdv_d128_kernel(
    const __hip_bfloat16* __restrict__ q, const __hip_bfloat16* __restrict__ k,
    const __hip_bfloat16* __restrict__ v, const __hip_bfloat16* __restrict__ dout,
    const float* __restrict__ lse, const float* __restrict__ delta,
    __hip_bfloat16* __restrict__ dk, __hip_bfloat16* __restrict__ dv, int BH, int H, int N,
    float scale, bool causal_arg, Strides sq, StridesGqa<kGqa> sk, Strides sv,
    StridesDoc<kDoc> sdo) {
  const bool causal = kDoc || causal_arg; // a document mask is causal by contract
  constexpr int kQStep = 32; // q rows per iteration (MFMA contraction width)
  __shared__ __hip_bfloat16 q_lds[2 * kImgElems]; // image dh: D columns 64dh..
  __shared__ __hip_bfloat16 do_lds[2 * kImgElems];
  __shared__ __hip_bfloat16 pt_lds_all[kWavesPerBlock][16][kPStride];
  __shared__ __hip_bfloat16 dst_lds_all[kWavesPerBlock][16][kPStride];

  const Coords tc = thread_coords();
  const int lane = tc.lane, wave = tc.wave, row16 = tc.row16, grp = tc.grp;
  const int st_row = tc.st_row, st_col = tc.st_col; // 0..31, 0..56
  __hip_bfloat16(*pt_lds)[kPStride] = pt_lds_all[wave];
  __hip_bfloat16(*dst_lds)[kPStride] = dst_lds_all[wave];
  const int st_t = vt_idx(st_row, st_col);

  const int nkb = (N + kBwdKeysPerBlock - 1) / kBwdKeysPerBlock;
  int group = 1; // kGqa: `bh` below counts (b, K/V head) pairs
  if constexpr (kGqa) group = sk.group;

  {
    const int bh = blockIdx.x / nkb; // gridDim.x == (BH / group) * nkb
    const int kb0 = (blockIdx.x - bh * nkb) * kBwdKeysPerBlock;
    const int j0 = kb0 + wave * 16; // this wave's 16 keys
    const bool valid = j0 < N;
    // q-side pointers of the group's first head (of THE head without kGqa)
    const __hip_bfloat16* qp = tslice(q, sq, bh * group, H);
    const __hip_bfloat16* kp = kv_slice(k, sk, bh * group, H, sk);
    const __hip_bfloat16* vp = kv_slice(v, sv, bh * group, H, sk);
    const __hip_bfloat16* dop = tslice(dout, sdo, bh * group, H);
    // lse / delta rows of that head: ONE offset for both tensors (a pointer
    // each, as in the D = 64 kernel, spills SGPRs in <kDoc, kGqa> here)
    int64_t stat0 = (int64_t)bh * group * N;

    bf16x8 kf[kKChunks128], vf2[kKChunks128];
    if (valid) {
      const int64_t kr = crow<kRagged>(j0 + row16, N);
#pragma unroll
      for (int c = 0; c < kKChunks128; ++c) {
        kf[c] = *(const bf16x8*)(kp + kr * sk.r + 32 * c + 8 * grp);
        vf2[c] = *(const bf16x8*)(vp + kr * sv.r + 32 * c + 8 * grp);
      }
    }

    f32x4 dv_acc[kDChunks128], dk_acc[kDChunks128]; // rows = key (4grp+r), cols = 16*db + row16
#pragma unroll
    for (int db = 0; db < kDChunks128; ++db) {
      dv_acc[db] = f32x4{0, 0, 0, 0};
      dk_acc[db] = f32x4{0, 0, 0, 0};
    }

    // i_start, the per-wave skip, the block-uniform kDoc break and the head
    // loop: see the D = 64 kernel.
    const int* dsp = nullptr;
    if constexpr (kDoc) dsp = sdo.doc_start + (int64_t)(bh * group / H) * N;
    const int i_start = causal ? (kb0 & ~(kQStep - 1)) : 0; // block-aligned diag
    int g = 0;
    do {
      int step_start = 0;
      if constexpr (kDoc) step_start = dstart(dsp, i_start, N);
      for (int i0 = i_start; i0 < N; i0 += kQStep) {
        if constexpr (kDoc) {
          if (step_start > kb0 + kBwdKeysPerBlock - 1) break;
          step_start = dstart(dsp, i0 + kQStep, N);
        }
        // ---- stage Q and dO into tiled images (two bf16x8 per thread) ----
        const int64_t st_g = crow<kRagged>(i0 + st_row, N);
#pragma unroll
        for (int dh = 0; dh < 2; ++dh) {
          *(bf16x8*)(&q_lds[dh * kImgElems + st_t]) =
              *(const bf16x8*)(qp + st_g * sq.r + 64 * dh + st_col);
          *(bf16x8*)(&do_lds[dh * kImgElems + st_t]) =
              *(const bf16x8*)(dop + st_g * sdo.r + 64 * dh + st_col);
        }
        decode_barrier();

        if (valid && (!causal || i0 + kQStep > j0)) {
          // two 16-q halves share this wave's key tile
#pragma unroll
          for (int hq = 0; hq < 2; ++hq) {
            const int q0 = i0 + 16 * hq; // this half's first q row
            const int qr = crow<kRagged>(q0 + row16, N);
            const float lse2_q = lse[stat0 + qr] * kLog2e; // log2 domain
            const float del_q = delta[stat0 + qr];
            int q_lo = 0, q_hi = 0;
            if constexpr (kDoc) {
              q_lo = dstart(dsp, q0 + row16, N);
              q_hi = (!kRagged || q0 + row16 < N) ? q0 + row16 : -1;
            }

            // ---- S^T = K Q^T, dP^T = V dO^T (rows = key, cols = q) ----
            f32x4 acc = {0, 0, 0, 0};
            f32x4 dpt = {0, 0, 0, 0};
#pragma unroll
            for (int c = 0; c < kKChunks128; ++c) {
              const int rm = (c >> 1) * kImgElems + vt_idx(16 * hq + row16, 32 * (c & 1) + 8 * grp);
              const bf16x8 qfr = *(const bf16x8*)(&q_lds[rm]);
              const bf16x8 dof = *(const bf16x8*)(&do_lds[rm]);
              acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(kf[c], qfr, acc, 0, 0, 0);
              dpt = __builtin_amdgcn_mfma_f32_16x16x32_bf16(vf2[c], dof, dpt, 0, 0, 0);
            }

            // ---- P^T and dS^T in C layout; write transposed slices ----
#pragma unroll
            for (int r = 0; r < 4; ++r) {
              const float p = bwd_prob<kRagged, kDoc>(acc[r], scale, lse2_q, j0 + 4 * grp + r,
                                                      q0 + row16, q_lo, q_hi, causal, N);
              const float ds = p * (dpt[r] - del_q) * scale;
              *(__bf16*)&pt_lds[4 * grp + r][16 * hq + row16] = (__bf16)p;
              *(__bf16*)&dst_lds[4 * grp + r][16 * hq + row16] = (__bf16)ds;
            }
          }

          // ---- dV += P^T @ dO ; dK += dS^T @ Q  (contraction over 32 q) ----
          const bf16x8 ptf = *(const bf16x8*)(&pt_lds[row16][8 * grp]);
          const bf16x8 dstf = *(const bf16x8*)(&dst_lds[row16][8 * grp]);
#pragma unroll
          for (int db = 0; db < kDChunks128; ++db) {
            const bf16x8 dob = read_tr_frag(do_lds + (db >> 2) * kImgElems, db & 3, lane);
            const bf16x8 qb = read_tr_frag(q_lds + (db >> 2) * kImgElems, db & 3, lane);
            dv_acc[db] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(ptf, dob, dv_acc[db], 0, 0, 0);
            dk_acc[db] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(dstf, qb, dk_acc[db], 0, 0, 0);
          }
        }
        decode_barrier(); // staged tiles consumed before restage
      }
      if constexpr (kGqa) {
        ++g;
        qp = tslice(q, sq, bh * group + g, H);
        dop = tslice(dout, sdo, bh * group + g, H);
        stat0 = (int64_t)(bh * group + g) * N;
      }
    } while (kGqa && g < group);

    if (valid) {
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int key_o = 4 * grp + r;
        if (kRagged && j0 + key_o >= N) continue;
        const int64_t row = ((int64_t)bh * N + j0 + key_o) * kAttnD128;
#pragma unroll
        for (int db = 0; db < kDChunks128; ++db) {
          ((__bf16*)dv)[row + 16 * db + row16] = (__bf16)dv_acc[db][r];
          ((__bf16*)dk)[row + 16 * db + row16] = (__bf16)dk_acc[db][r];
        }
      }
    }
  }
}

// ------------------------------------------------------------------- dQ
// The D = 64 kernel's split: a wave owns 16 q rows, the block 64, and 32-key
// tiles stream past: K as two images (read row-major for S^T, transposed for
// dS K), V row-major at stride 136. Two pieces per thread and tensor.
template <bool kRagged, bool kDoc, bool kGqa>
kD128Fn __global__ void __launch_bounds__(kAttnThreads) attn_bwd_dq_d128_kernel(
    const __hip_bfloat16* __restrict__ q, const __hip_bfloat16* __restrict__ k,
    const __hip_bfloat16* __restrict__ v, const __hip_bfloat16* __restrict__ dout,
    const float* __restrict__ lse, const float* __restrict__ delta,
    __hip_bfloat16* __restrict__ dq, int BH, int H, int N, float scale, bool causal_arg,
    Strides sq, StridesGqa<kGqa> sk, Strides sv, StridesDoc<kDoc> sdo) {
  const bool causal = kDoc || causal_arg; // a document mask is causal by contract
  __shared__ __hip_bfloat16 k_lds[2 * kImgElems]; // image dh: D columns 64dh..
  __shared__ __hip_bfloat16 v_lds[kKT][kKVStrideD128];
  __shared__ __hip_bfloat16 ds_lds_all[kWavesPerBlock][kQT][kPStride]; // [q][key32]

  const Coords tc = thread_coords();
  const int lane = tc.lane, wave = tc.wave, row16 = tc.row16, grp = tc.grp;
  const int st_row = tc.st_row, st_col = tc.st_col; // 0..31, 0..56
  __hip_bfloat16(*ds_lds)[kPStride] = ds_lds_all[wave];
  const int st_t = vt_idx(st_row, st_col);

  const int nqb = (N + kDqRowsPerBlock - 1) / kDqRowsPerBlock;
  const int64_t total_blocks = (int64_t)BH * nqb;

  for (int64_t blk = blockIdx.x; blk < total_blocks; blk += gridDim.x) {
    const int bh = blk / nqb;
    const int qb0 = (blk - (int64_t)bh * nqb) * kDqRowsPerBlock;
    const int i0 = qb0 + wave * kQT;
    const bool valid = i0 < N;
    const __hip_bfloat16* qp = tslice(q, sq, bh, H);
    const __hip_bfloat16* kp = kv_slice(k, sk, bh, H, sk);
    const __hip_bfloat16* vp = kv_slice(v, sv, bh, H, sk);
    const __hip_bfloat16* dop = tslice(dout, sdo, bh, H);
    const float* lsep = lse + (int64_t)bh * N;
    const float* delp = delta + (int64_t)bh * N;

    bf16x8 qf[kKChunks128], dof[kKChunks128];
    float lse_q = 0.0f, del_q = 0.0f;
    if (valid) {
      const int64_t qr = crow<kRagged>(i0 + row16, N);
#pragma unroll
      for (int c = 0; c < kKChunks128; ++c) {
        qf[c] = *(const bf16x8*)(qp + qr * sq.r + 32 * c + 8 * grp);
        dof[c] = *(const bf16x8*)(dop + qr * sdo.r + 32 * c + 8 * grp);
      }
      lse_q = lsep[qr] * kLog2e; // log2 domain
      del_q = delp[qr];
    }

    f32x4 dq_acc[kDChunks128];
#pragma unroll
    for (int db = 0; db < kDChunks128; ++db) dq_acc[db] = f32x4{0, 0, 0, 0};

    // the key walk, its ends and the kDoc skips: see the D = 64 kernel
    const int kv_end_block = causal ? min(qb0 + kDqRowsPerBlock, N) : N;
    const int my_kv_end = causal ? (i0 + kQT) : N;
    int j_begin = 0, q_lo = 0, q_hi = 0, wave_start = 0;
    if constexpr (kDoc) {
      const int* dsp = sdo.doc_start + (int64_t)(bh / H) * N;
      j_begin = dstart(dsp, qb0, N) & ~(kKT - 1);
      q_lo = dstart(dsp, i0 + row16, N);
      q_hi = (!kRagged || i0 + row16 < N) ? i0 + row16 : -1;
      wave_start = __builtin_amdgcn_readfirstlane(dstart(dsp, i0, N));
    }

    for (int j0 = j_begin; j0 < kv_end_block; j0 += kKT) {
      const int64_t st_g = crow<kRagged>(j0 + st_row, N);
#pragma unroll
      for (int dh = 0; dh < 2; ++dh) {
        *(bf16x8*)(&k_lds[dh * kImgElems + st_t]) =
            *(const bf16x8*)(kp + st_g * sk.r + 64 * dh + st_col);
        *(bf16x8*)(&v_lds[st_row][64 * dh + st_col]) =
            *(const bf16x8*)(vp + st_g * sv.r + 64 * dh + st_col);
      }
      decode_barrier();

      if (valid && j0 < my_kv_end && (!kDoc || j0 + kKT > wave_start)) {
#pragma unroll
        for (int h = 0; h < 2; ++h) { // two 16-key halves
          // S^T rows = key (4grp+r), col = q (row16)
          f32x4 acc = {0, 0, 0, 0};
          f32x4 dpt = {0, 0, 0, 0};
#pragma unroll
          for (int c = 0; c < kKChunks128; ++c) {
            const bf16x8 kfr = *(const bf16x8*)(&k_lds[(c >> 1) * kImgElems +
                                                       vt_idx(16 * h + row16, 32 * (c & 1) + 8 * grp)]);
            const bf16x8 vfr = *(const bf16x8*)(&v_lds[16 * h + row16][32 * c + 8 * grp]);
            acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(kfr, qf[c], acc, 0, 0, 0);
            dpt = __builtin_amdgcn_mfma_f32_16x16x32_bf16(vfr, dof[c], dpt, 0, 0, 0);
          }
          // dS^T -> [q][key] slice (4 consecutive keys pack per write)
          bf16x4 dsw;
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            const float p = bwd_prob<kRagged, kDoc>(acc[r], scale, lse_q,
                                                    j0 + 16 * h + 4 * grp + r, i0 + row16, q_lo,
                                                    q_hi, causal, N);
            dsw[r] = (__bf16)(p * (dpt[r] - del_q) * scale);
          }
          *(bf16x4*)(&ds_lds[row16][16 * h + 4 * grp]) = dsw;
        }

        // ---- dq += dS @ K (contraction over the 32 keys) ----
        const bf16x8 dsf = *(const bf16x8*)(&ds_lds[row16][8 * grp]);
#pragma unroll
        for (int db = 0; db < kDChunks128; ++db) {
          const bf16x8 kb = read_tr_frag(k_lds + (db >> 2) * kImgElems, db & 3, lane);
          dq_acc[db] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(dsf, kb, dq_acc[db], 0, 0, 0);
        }
      }
      decode_barrier();
    }

    if (valid) {
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int q_o = 4 * grp + r;
        if (kRagged && i0 + q_o >= N) continue;
        __bf16* qrow = (__bf16*)dq + ((int64_t)bh * N + i0 + q_o) * kAttnD128;
#pragma unroll
        for (int db = 0; db < kDChunks128; ++db) qrow[16 * db + row16] = (__bf16)dq_acc[db][r];
      }
    }
  }
}

// ---------------------------------------------------------------- launchers
// The form of the forward that runs (see the kernel's comment).
constexpr int kFwdSubsD128 = 1;
constexpr int kFwdRowsPerBlockD128 = kWavesPerBlock * kFwdSubsD128 * kQT;

static void attn_fwd_d128(const at::Tensor& q, const at::Tensor& k, const at::Tensor& v,
                          at::Tensor& o, at::Tensor& lse, double scale, bool causal,
                          const int* dsp, int G) {
  const int H = q.size(1), N = q.size(2), BH = q.size(0) * H;
  auto stream = c10::hip::getCurrentHIPStream();
  static_assert(kKTF % (kFwdSubsD128 * kQT) == 0); // a wave's q rows also end at N then
  with_variant(N % kKTF != 0, dsp != nullptr, G > 1, [&](auto ragged, auto doc, auto gqa) {
    constexpr bool kDoc = decltype(doc)::value, kGqa = decltype(gqa)::value;
    hipLaunchKernelGGL(
        (attn_fwd_d128_kernel<kFwdSubsD128, decltype(ragged)::value, kDoc, kGqa>),
        dim3(attn_grid(BH, N, kFwdRowsPerBlockD128)), dim3(kAttnThreads), 0, stream,
        (const __hip_bfloat16*)q.data_ptr(), (const __hip_bfloat16*)k.data_ptr(),
        (const __hip_bfloat16*)v.data_ptr(), (__hip_bfloat16*)o.data_ptr(), lse.data_ptr<float>(),
        BH, H, N, (float)scale, causal, strides_of(q), gqa_strides_of<kGqa>(k, G),
        doc_strides_of<kDoc>(v, dsp));
  });
}

static void attn_bwd_d128(const at::Tensor& q, const at::Tensor& k, const at::Tensor& v,
                          const at::Tensor& dout, const at::Tensor& o, const at::Tensor& lse,
                          at::Tensor& dq, at::Tensor& dk, at::Tensor& dv, at::Tensor& delta,
                          double scale, bool causal, const int* dsp, int G) {
  const int H = q.size(1), N = q.size(2), BH = q.size(0) * H;
  auto stream = c10::hip::getCurrentHIPStream();
  const int64_t rows = (int64_t)BH * N;
  hipLaunchKernelGGL(attn_bwd_delta_d128_kernel, dim3(grid_for(rows * 16, kBlock)), dim3(kBlock),
                     0, stream, (const __hip_bfloat16*)dout.data_ptr(),
                     (const __hip_bfloat16*)o.data_ptr(), delta.data_ptr<float>(), rows, H, N,
                     strides_of(dout));
  const bool ragged = N % kBwdKeysPerBlock != 0 || N % kDqRowsPerBlock != 0;
  with_variant(ragged, dsp != nullptr, G > 1, [&](auto ragged_c, auto doc, auto gqa) {
    constexpr bool kRagged = decltype(ragged_c)::value, kDoc = decltype(doc)::value,
                   kGqa = decltype(gqa)::value;
    auto launch = [&](auto kernel, int grid, auto... outputs) {
      hipLaunchKernelGGL(kernel, dim3(grid), dim3(kAttnThreads), 0, stream, (const __hip_bfloat16*)q.data_ptr(),
                         (const __hip_bfloat16*)k.data_ptr(), (const __hip_bfloat16*)v.data_ptr(),
                         (const __hip_bfloat16*)dout.data_ptr(), lse.data_ptr<float>(),
                         delta.data_ptr<float>(), outputs..., BH, H, N, (float)scale, causal,
                         strides_of(q), gqa_strides_of<kGqa>(k, G), strides_of(v),
                         doc_strides_of<kDoc>(dout, dsp));
    };
    // dK/dV: one block per (b, K/V head, key block), all of them (no cap)
    const int64_t dkdv_blocks =
        (int64_t)(BH / G) * ((N + kBwdKeysPerBlock - 1) / kBwdKeysPerBlock);
    TORCH_CHECK(dkdv_blocks <= INT32_MAX, "attn_bwd: B * Hkv * ceil(N / 64) too large");
    launch(attn_bwd_dkdv_d128_kernel<kRagged, kDoc, kGqa>, (int)dkdv_blocks,
           (__hip_bfloat16*)dk.data_ptr(), (__hip_bfloat16*)dv.data_ptr());
    launch(attn_bwd_dq_d128_kernel<kRagged, kDoc, kGqa>, attn_grid(BH, N, kDqRowsPerBlock),
           (__hip_bfloat16*)dq.data_ptr());
  });
}
