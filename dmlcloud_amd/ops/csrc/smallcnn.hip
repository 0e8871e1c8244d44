// Fused conv3x3(pad1) + ReLU + maxpool2x2 kernels for gfx950 (MI355X).
//
// Motivation (profiles/mnist_b1024_eager_kernel_stats.md): MIOpen executes
// the benchmark MNIST-CNN as im2col + hundreds of small batched GEMMs per
// step plus a pathological find phase. The model's tensors are tiny, so
// the MI355X-native design stages whole per-sample planes in LDS and
// computes each layer in ONE kernel per direction.
//
// Iteration history (each measured with rocprofv3 / cuda events on MI355X;
// numbers are the conv2 shape [16ch 14x14] at batch 16384):
//   v1  one thread per output, global scalar loads -> cache-amplified.
//   v2  LDS-staged per-sample workgroups           -> bwd_weight-dominated.
//   v3  halo-padded planes (branch-free taps), bank-skewed strides,
//       chunked bwd_weight: fwd 1439us / bwd_data 1199us / bwd_w 914us.
//   v4  instruction-count pass: fwd computes a 2x2 POOLED block per thread
//       from a 6x6 window read as ds_read_b128+b64 rows; bwd_data a 2x4 din
//       block from a 4x6 dconv window; bwd_weight reads a dense per-cell
//       (g, offset) pair + 9 taps. Padded geometry keeps every vector read
//       16B-aligned and channel strides bank-skewed (mod 64 != 0).
//   v4+ bwd_weight ends in one row of partials per workgroup and an ordered
//       second-stage sum: run-to-run reproducible gradients
//       (profiles/smallcnn_bwdw_ordered_partials.md).
//   v6  (this file) conv2-like layers run fwd and bwd_data as f32 MFMA
//       implicit GEMMs, bit for bit the VALU kernels' results
//       (profiles/smallcnn_mfma.md); see "f32 MFMA forms" below.
//   v7  conv2 bwd_weight (COUT == CIN == 16) is an f32 MFMA implicit GEMM
//       too: the dense form of the pool gradient does 4x the gather's
//       multiplications and is still faster, bit for bit the VALU
//       kernel's chains (profiles/smallcnn_bwdw_mfma.md); see
//       conv3x3_relu_pool_bwd_weight_mfma_kernel.
//   v8  conv2 bwd_data and conv1 bwd_weight are one kernel when conv1 needs
//       no input gradient: conv2's din, whose only reader was conv1
//       bwd_weight, goes from the MFMA accumulators through LDS into the
//       gather and never to memory, bit for bit the two kernels
//       (profiles/smallcnn_bwd_merged.md); see
//       conv3x3_relu_pool_bwd_data_weight_kernel.
//   v5  data-movement pass, arithmetic untouched
//       (profiles/smallcnn_pipelined.md):
//       - the ReLU gate travels in bit 2 of the argmax byte, so neither
//         backward kernel reads `pooled`;
//       - staging is sample-invariant: every thread works out ONCE which
//         16-byte pieces of a sample it owns and where they land in LDS,
//         so the per-sample loop has no division and loads float4 /
//         packed argmax words (scalar loads when a base is unaligned);
//       - loads of a sample are issued together, up to four float4 per
//         thread in flight, before any of them is written to LDS. Issuing
//         them one sample ahead, before the math, was built and measured:
//         faster per kernel at the conv1 shapes, but in the full step
//         faster on one box and slower and erratic on another, so the
//         sample loop stays fill -> barrier -> math -> barrier;
//       - bwd_data writes all four positions of each pooled cell instead
//         of re-zeroing its plane, and stores din as 8-byte pairs;
//       - the reduce kernel stores dw/db instead of adding to them.
//
// ReLU/maxpool tie-breaking matches torch: first index wins ties, and a
// pooled value of exactly 0 (all-negative window) propagates no gradient.
//
// The argmax byte is private to these kernels: bits 0-1 = position of the
// maximum inside the 2x2 window (row-major), bit 2 = "gated" (pooled value
// not > 0, no gradient).

#include <torch/extension.h>
#include <c10/hip/HIPStream.h>

#include "ops_common.h"

namespace dmlamd {

typedef float f4 __attribute__((ext_vector_type(4)));
typedef float f2 __attribute__((ext_vector_type(2)));

constexpr int kGateBit = 4;

// Padded plane geometry. Guard covers the 6x6 (fwd) / 4x6 (bwd) window
// over-read of ragged 2x-blocks; PADW is a multiple of 4 so row starts at
// 4-aligned x are 16B-aligned; cstride keeps 4-alignment and avoids
// cstride % 64 == 0 (cross-channel bank collisions).
struct PlaneGeom {
  int PADH, PADW, cs;
};

__host__ __device__ __forceinline__ PlaneGeom plane_geom(int H, int W) {
  PlaneGeom g;
  const int PH = H / 2, PW = W / 2;
  g.PADH = H + 2 + ((PH & 1) ? 2 : 0);
  int padw = W + 2 + ((PW & 1) ? 2 : 0);
  g.PADW = (padw + 3) & ~3;
  g.cs = g.PADH * g.PADW;
  // keep cs a multiple of 4 (16B-aligned rows) with cs/4 odd, so the
  // per-channel bank offset (cs mod 64) has gcd(cs,64)=4 and 16
  // simultaneous cross-channel b32 reads at equal (y,x) span 16 distinct
  // banks (measured: cs=360 aliased ci and ci+8 -> 5.2 conflict
  // cycles/LDS instruction in bwd_weight, profiles/smallcnn_pmc.txt)
  if ((g.cs & 7) == 0) g.cs += 4; // cs is a multiple of 4 by construction
  return g;
}

__host__ __device__ __forceinline__ int pooled_stride(int pcells) {
  return pcells + ((pcells % 64) ? 0 : 4) + 1; // bank skew
}

__device__ __forceinline__ void stage_to_lds(const float* __restrict__ g, float* __restrict__ l,
                                             int count) {
  for (int i = threadIdx.x; i < count; i += kBlock) l[i] = g[i];
}

// Read 6 consecutive padded floats at a 16B-aligned offset.
__device__ __forceinline__ void read_row6(const float* __restrict__ p, float* __restrict__ row) {
  const f4 a = *(const f4*)p;
  const f2 b = *(const f2*)(p + 4);
  row[0] = a.x;
  row[1] = a.y;
  row[2] = a.z;
  row[3] = a.w;
  row[4] = b.x;
  row[5] = b.y;
}

// ------------------------------------------------------- sample staging
//
// A sample's input plane is CIN*H*W contiguous floats, a multiple of 4
// because H and W are even. It is cut into float4 pieces; thread t owns
// pieces t, t + kBlock, ... The first PF of them are loaded into registers
// together and then written to LDS, so their latencies overlap; pieces
// beyond PF * kBlock, which only shapes larger than the MNIST ones have,
// are copied one by one. Where a piece
// lands in the padded LDS plane does not depend on the sample, so it is
// worked out once per thread: o0 for elements 0-1, o1 for elements 2-3 (a
// piece may straddle a row end, a pair cannot: W is even).

__device__ __forceinline__ void plane_piece_offsets(int piece, int H, int W, const PlaneGeom& pg,
                                                    int& o0, int& o1) {
  const int e = 4 * piece, plane = H * W;
  int ci = e / plane;
  const int rem = e - ci * plane;
  int y = rem / W;
  int x = rem - y * W;
  o0 = ci * pg.cs + (y + 1) * pg.PADW + (x + 1);
  x += 2;
  if (x == W) {
    x = 0;
    if (++y == H) {
      y = 0;
      ++ci;
    }
  }
  o1 = ci * pg.cs + (y + 1) * pg.PADW + (x + 1);
}

__device__ __forceinline__ f4 load4(const float* __restrict__ p, bool vec) {
  if (vec) return *(const f4*)p;
  f4 r;
  r.x = p[0];
  r.y = p[1];
  r.z = p[2];
  r.w = p[3];
  return r;
}

__device__ __forceinline__ void put_piece(float* __restrict__ lds, int o0, int o1, const f4 v) {
  lds[o0] = v.x;
  lds[o0 + 1] = v.y;
  lds[o1] = v.z;
  lds[o1 + 1] = v.w;
}

template <int PF>
struct PlaneStage {
  f4 v[PF];
  int o0[PF], o1[PF];

  __device__ __forceinline__ void init(int npieces, int H, int W, const PlaneGeom& pg) {
#pragma unroll
    for (int k = 0; k < PF; ++k) {
      const int piece = threadIdx.x + k * kBlock;
      o0[k] = o1[k] = 0;
      if (piece < npieces) plane_piece_offsets(piece, H, W, pg, o0[k], o1[k]);
    }
  }
  // issue the global loads of one sample's plane `g`
  __device__ __forceinline__ void load(const float* __restrict__ g, int npieces, bool vec) {
#pragma unroll
    for (int k = 0; k < PF; ++k) {
      const int piece = threadIdx.x + k * kBlock;
      if (piece < npieces) v[k] = load4(g + 4 * piece, vec);
    }
  }
  // write the loaded plane into the padded LDS region (halo stays zero)
  __device__ __forceinline__ void store(const float* __restrict__ g, float* __restrict__ lds,
                                        int npieces, bool vec, int H, int W,
                                        const PlaneGeom& pg) const {
#pragma unroll
    for (int k = 0; k < PF; ++k) {
      const int piece = threadIdx.x + k * kBlock;
      if (piece < npieces) put_piece(lds, o0[k], o1[k], v[k]);
    }
    for (int piece = threadIdx.x + PF * kBlock; piece < npieces; piece += kBlock) {
      int a, b;
      plane_piece_offsets(piece, H, W, pg, a, b);
      put_piece(lds, a, b, load4(g + 4 * piece, vec));
    }
  }
};

// A sample's pooled-side tensors (dpooled fp32, argmax bytes) hold
// `cells` = COUT*PH*PW elements, cut into groups of 4 consecutive cells;
// thread t owns groups t, t + kBlock, ... Each cell has a sample-invariant
// integer `code` telling the kernel where it goes in LDS (worked out once
// per thread, -1 for the cells past the end of a ragged last group). With
// cells % 4 == 0 and aligned bases a group is one float4 and one 32-bit
// word of argmax bytes; otherwise it is loaded cell by cell.
template <int PF>
struct CellStage {
  f4 g[PF];
  uint32_t a[PF];
  int code[PF][4];

  template <typename CodeFn>
  __device__ __forceinline__ void init(int cells, CodeFn code_of) {
#pragma unroll
    for (int k = 0; k < PF; ++k) {
      const int c0 = 4 * (threadIdx.x + k * kBlock);
#pragma unroll
      for (int j = 0; j < 4; ++j) code[k][j] = (c0 + j < cells) ? code_of(c0 + j) : -1;
    }
  }
  static __device__ __forceinline__ void load_group(const float* __restrict__ dp,
                                                    const uint8_t* __restrict__ am, int c0,
                                                    int cells, bool vec, f4& gv, uint32_t& av) {
    if (vec) {
      gv = *(const f4*)(dp + c0);
      av = *(const uint32_t*)(am + c0);
    } else {
      float t[4];
      av = 0;
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const bool ok = c0 + j < cells;
        t[j] = ok ? dp[c0 + j] : 0.0f;
        av |= (ok ? (uint32_t)am[c0 + j] : (uint32_t)kGateBit) << (8 * j);
      }
      gv.x = t[0];
      gv.y = t[1];
      gv.z = t[2];
      gv.w = t[3];
    }
  }
  // dp / am point at the sample's first cell
  __device__ __forceinline__ void load(const float* __restrict__ dp,
                                       const uint8_t* __restrict__ am, int cells, bool vec) {
#pragma unroll
    for (int k = 0; k < PF; ++k) {
      const int c0 = 4 * (threadIdx.x + k * kBlock);
      if (c0 < cells) load_group(dp, am, c0, cells, vec, g[k], a[k]);
    }
  }
  // put(code, gradient, argmax byte) places one cell in LDS
  template <typename CodeFn, typename PutFn>
  __device__ __forceinline__ void store(const float* __restrict__ dp,
                                        const uint8_t* __restrict__ am, int cells, bool vec,
                                        CodeFn code_of, PutFn put) const {
#pragma unroll
    for (int k = 0; k < PF; ++k) {
      const int c0 = 4 * (threadIdx.x + k * kBlock);
      if (c0 < cells) {
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          if (code[k][j] >= 0) put(code[k][j], g[k][j], (a[k] >> (8 * j)) & 0xffu);
        }
      }
    }
    for (int c0 = 4 * (threadIdx.x + PF * kBlock); c0 < cells; c0 += 4 * kBlock) {
      f4 gv;
      uint32_t av;
      load_group(dp, am, c0, cells, vec, gv, av);
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        if (c0 + j < cells) put(code_of(c0 + j), gv[j], (av >> (8 * j)) & 0xffu);
      }
    }
  }
};

// --------------------------------------------------------------- forward

// Workgroup = one sample (grid-stride). Thread = (co, 2x2 pooled block).
// LDS: [CIN][cs] halo-padded input + [COUT*CIN*9] weights + [COUT] bias.
// Pooled values and argmax bytes are stored straight from the math loop;
// collecting them in LDS for 16-byte stores measured 1-2% slower
// (profiles/smallcnn_pipelined.md).
//
// VEC = true is the build for 16-byte-aligned bases; VEC = false decides
// between vector and scalar loads by the run-time flag.
template <int PF, bool VEC>
__global__ void __launch_bounds__(kBlock) conv3x3_relu_pool_fwd_kernel(
    const float* __restrict__ in, const float* __restrict__ w, const float* __restrict__ bias,
    float* __restrict__ out, uint8_t* __restrict__ argmax, int N, int CIN, int COUT, int H,
    int W, int in_vec_flag) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const bool in_vec = VEC || in_vec_flag;
  const PlaneGeom pg = plane_geom(H, W);
  const int PH = H / 2, PW = W / 2;
  const int ocells = COUT * PH * PW;
  float* ilds = (float*)smem; // [CIN][cs]
  float* wlds = ilds + CIN * pg.cs; // [COUT][CIN][9]
  float* blds = wlds + COUT * CIN * 9; // [COUT]

  const int plane = CIN * H * W;
  const int npieces = plane / 4;
  const int BH = (PH + 1) / 2, BW = (PW + 1) / 2; // 2x2 pooled blocks
  const int nblocks = COUT * BH * BW;

  PlaneStage<PF> st;
  st.init(npieces, H, W, pg);
  int n = blockIdx.x; // the launcher guarantees gridDim.x <= N
  st.load(in + (int64_t)n * plane, npieces, in_vec);

  stage_to_lds(w, wlds, COUT * CIN * 9);
  stage_to_lds(bias, blds, COUT);
  for (int i = threadIdx.x; i < CIN * pg.cs; i += kBlock) ilds[i] = 0.0f; // halo, once
  __syncthreads();
  st.store(in + (int64_t)n * plane, ilds, npieces, in_vec, H, W, pg);
  __syncthreads();

  for (; n < N; n += gridDim.x) {
    const int nn = n + gridDim.x;
    float* outn = out + (int64_t)n * ocells;
    uint8_t* argn = argmax + (int64_t)n * ocells;

    for (int t = threadIdx.x; t < nblocks; t += kBlock) {
      const int bx = t % BW;
      const int by = (t / BW) % BH;
      const int co = t / (BW * BH);
      const int y0 = 4 * by, x0 = 4 * bx; // padded top-left of 6x6 window

      float conv[4][4];
      const float bz = blds[co];
#pragma unroll
      for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) conv[i][j] = bz;

      const float* wc = wlds + co * CIN * 9;
      for (int ci = 0; ci < CIN; ++ci) {
        const float* ip = ilds + ci * pg.cs + y0 * pg.PADW + x0;
        float win[6][6];
#pragma unroll
        for (int r = 0; r < 6; ++r) read_row6(ip + r * pg.PADW, win[r]);
        const float* wk = wc + ci * 9;
#pragma unroll
        for (int ky = 0; ky < 3; ++ky) {
#pragma unroll
          for (int kx = 0; kx < 3; ++kx) {
            const float wv = wk[ky * 3 + kx];
#pragma unroll
            for (int cy = 0; cy < 4; ++cy) {
#pragma unroll
              for (int cx = 0; cx < 4; ++cx) {
                conv[cy][cx] = fmaf(wv, win[cy + ky][cx + kx], conv[cy][cx]);
              }
            }
          }
        }
      }

      // relu + 2x2 max per pooled cell; first index wins ties
#pragma unroll
      for (int dy = 0; dy < 2; ++dy) {
        const int py = 2 * by + dy;
        if (py >= PH) break;
#pragma unroll
        for (int dx = 0; dx < 2; ++dx) {
          const int px = 2 * bx + dx;
          if (px >= PW) continue;
          const float r0 = fmaxf(conv[2 * dy][2 * dx], 0.0f);
          const float r1 = fmaxf(conv[2 * dy][2 * dx + 1], 0.0f);
          const float r2 = fmaxf(conv[2 * dy + 1][2 * dx], 0.0f);
          const float r3 = fmaxf(conv[2 * dy + 1][2 * dx + 1], 0.0f);
          float m = r0;
          int arg = 0;
          if (r1 > m) { m = r1; arg = 1; }
          if (r2 > m) { m = r2; arg = 2; }
          if (r3 > m) { m = r3; arg = 3; }
          if (!(m > 0.0f)) arg |= kGateBit;
          const int cell = (co * PH + py) * PW + px;
          outn[cell] = m;
          argn[cell] = (uint8_t)arg;
        }
      }
    }
    __syncthreads(); // math done: ilds may be overwritten

    if (nn < N) {
      st.load(in + (int64_t)nn * plane, npieces, in_vec);
      st.store(in + (int64_t)nn * plane, ilds, npieces, in_vec, H, W, pg);
    }
    __syncthreads(); // next plane published
  }
}

// ------------------------------------------------------------- bwd data

// Workgroup = one sample. Thread = (ci, 2x4 din block): reads a 4x6
// dconv window per cout (vectorized rows), 8 outputs per thread.
// The relu+maxpool-folded conv gradient of a sample sits in a halo-padded
// LDS plane. Every pooled cell writes all four positions of its 2x2 window
// (the gradient at the argmax position unless gated, zero elsewhere), so
// the interior is fully rewritten per sample and only the halo is zeroed,
// once.
template <int PF, bool VEC>
__global__ void __launch_bounds__(kBlock) conv3x3_relu_pool_bwd_data_kernel(
    const float* __restrict__ dpooled, const uint8_t* __restrict__ argmax,
    const float* __restrict__ w, float* __restrict__ din, int N, int CIN, int COUT, int H,
    int W, int cell_vec_flag, int din_vec_flag) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const bool cell_vec = VEC || cell_vec_flag, din_vec = VEC || din_vec_flag;
  const PlaneGeom pg = plane_geom(H, W);
  float* dclds = (float*)smem; // [COUT][cs]
  float* wlds = dclds + COUT * pg.cs; // [COUT][CIN][9]

  const int PH = H / 2, PW = W / 2;
  const int pcells = PH * PW;
  const int cells = COUT * pcells;
  const int BH = H / 2, BW = (W + 3) / 4; // 2x4 output blocks
  const int nblocks = CIN * BH * BW;

  // code = LDS offset of the top-left position of the cell's 2x2 window
  auto code_of = [&](int cell) {
    const int co = cell / pcells;
    const int rem = cell - co * pcells;
    const int py = rem / PW, px = rem - py * PW;
    return co * pg.cs + (2 * py + 1) * pg.PADW + (2 * px + 1);
  };
  auto put = [&](int code, float g, uint32_t a) {
    const float v = (a & kGateBit) ? 0.0f : g;
    const uint32_t sub = a & 3u;
    dclds[code] = (sub == 0) ? v : 0.0f;
    dclds[code + 1] = (sub == 1) ? v : 0.0f;
    dclds[code + pg.PADW] = (sub == 2) ? v : 0.0f;
    dclds[code + pg.PADW + 1] = (sub == 3) ? v : 0.0f;
  };

  CellStage<PF> st;
  st.init(cells, code_of);
  int n = blockIdx.x; // the launcher guarantees gridDim.x <= N
  st.load(dpooled + (int64_t)n * cells, argmax + (int64_t)n * cells, cells, cell_vec);

  stage_to_lds(w, wlds, COUT * CIN * 9);
  for (int i = threadIdx.x; i < COUT * pg.cs; i += kBlock) dclds[i] = 0.0f; // halo, once
  __syncthreads();
  st.store(dpooled + (int64_t)n * cells, argmax + (int64_t)n * cells, cells, cell_vec, code_of,
           put);
  __syncthreads();

  for (; n < N; n += gridDim.x) {
    const int nn = n + gridDim.x;

    for (int t = threadIdx.x; t < nblocks; t += kBlock) {
      const int bx = t % BW;
      const int by = (t / BW) % BH;
      const int ci = t / (BW * BH);
      const int y0 = 2 * by, x0 = 4 * bx; // din block top-left (unpadded)

      float acc[2][4] = {{0, 0, 0, 0}, {0, 0, 0, 0}};
      for (int co = 0; co < COUT; ++co) {
        // dconv rows y0-1..y0+2 -> padded rows y0..y0+3; cols x0-1..x0+4
        // -> padded cols x0..x0+5 (aligned: x0 multiple of 4)
        const float* dp = dclds + co * pg.cs + y0 * pg.PADW + x0;
        float win[4][6];
#pragma unroll
        for (int r = 0; r < 4; ++r) read_row6(dp + r * pg.PADW, win[r]);
        const float* wk = wlds + (co * CIN + ci) * 9;
        // din(y,x) += w[ky][kx] * dconv(y-ky+1, x-kx+1)
        // local: dconv(y0+dy-ky+1, x0+dx-kx+1) = win[dy-ky+2][dx-kx+2]
#pragma unroll
        for (int ky = 0; ky < 3; ++ky) {
#pragma unroll
          for (int kx = 0; kx < 3; ++kx) {
            const float wv = wk[ky * 3 + kx];
#pragma unroll
            for (int dy = 0; dy < 2; ++dy) {
#pragma unroll
              for (int dx = 0; dx < 4; ++dx) {
                acc[dy][dx] = fmaf(wv, win[dy - ky + 2][dx - kx + 2], acc[dy][dx]);
              }
            }
          }
        }
      }
      // W and x0 are even, so each pair of columns is inside the row or
      // outside it as a whole and starts at an even element
#pragma unroll
      for (int dy = 0; dy < 2; ++dy) {
        float* drow = din + (((int64_t)n * CIN + ci) * H + y0 + dy) * W + x0;
#pragma unroll
        for (int dx = 0; dx < 4; dx += 2) {
          if (x0 + dx < W) {
            if (din_vec) {
              f2 v;
              v.x = acc[dy][dx];
              v.y = acc[dy][dx + 1];
              *(f2*)(drow + dx) = v;
            } else {
              drow[dx] = acc[dy][dx];
              drow[dx + 1] = acc[dy][dx + 1];
            }
          }
        }
      }
    }
    __syncthreads(); // math done: dclds may be overwritten
    if (nn < N) {
      st.load(dpooled + (int64_t)nn * cells, argmax + (int64_t)nn * cells, cells, cell_vec);
      st.store(dpooled + (int64_t)nn * cells, argmax + (int64_t)nn * cells, cells, cell_vec,
               code_of, put);
    }
    __syncthreads();
  }
}

// ------------------------------------------- f32 MFMA forms (16 channels)
//
// conv2-like layers (COUT == 16, CIN in {4, 8, 12, 16}) run forward and
// bwd_data as an implicit GEMM per sample on v_mfma_f32_16x16x4_f32. The
// instruction is a k-ordered f32 fmaf chain, so with k in the order of the
// loops above the results are bit for bit those of the VALU kernels; it
// issues at the VALU's peak rate from one VGPR per operand and pads a 14x14
// plane to 13 tiles of 16 rows (6 %) where the 4x4 blocks pad it to 16x16
// (31 %). Staging, the padded planes and the sample loop are those of the
// VALU kernels.
//
// Lane l supplies A[row l&15][k = 4s + (l>>4)] and B[k = 4s + (l>>4)][l&15]
// at step s, and holds D[rows 4*(l>>4) .. +3][column l&15]. A row's operand
// is one LDS word at (row's top-left offset, from a per-workgroup table) +
// (k's offset inside the 3x3xC stencil). k = c*9 + tap, so step s+9 is step
// s four channels on: nine per-lane k-offsets and a uniform stride suffice.
// B is stored as [k][16], which makes a step's operand word 64*s + lane.
//
// Wave v owns tiles v, v+4, ... and runs up to three of them as interleaved
// accumulator chains sharing B (a dependent MFMA has 40 cycles of latency
// against 32 of issue). At 13 tiles that is 3+1 tiles for wave 0 and 3 for
// the others. Measured at the conv2 shape (profiles/smallcnn_mfma.md):
// three chains beat one, two and four; rotating the wave that carries the
// odd tile with the sample index, and loading the next sample ahead of the
// math, gained nothing.

constexpr int kMfmaChains = 3;

template <int NC>
__device__ __forceinline__ void mfma_chains(const float* __restrict__ alds,
                                            const float* __restrict__ wbl,
                                            const int (&base)[kMfmaChains], const int (&koff)[9],
                                            int groups, int gstride, f4 (&acc)[kMfmaChains]) {
  for (int cg = 0; cg < groups; ++cg) {
    const float* ap = alds + cg * gstride;
    const float* bp = wbl + cg * 9 * kWave;
#pragma unroll
    for (int s = 0; s < 9; ++s) {
      const float b = bp[s * kWave];
#pragma unroll
      for (int i = 0; i < NC; ++i) {
        acc[i] = __builtin_amdgcn_mfma_f32_16x16x4f32(ap[base[i] + koff[s]], b, acc[i], 0, 0, 0);
      }
    }
  }
}

// acc[i] += A(tile of base[i]) x B for the first nc (wave-uniform) chains
__device__ __forceinline__ void mfma_tiles(int nc, const float* __restrict__ alds,
                                           const float* __restrict__ wbl,
                                           const int (&base)[kMfmaChains], const int (&koff)[9],
                                           int groups, int gstride, f4 (&acc)[kMfmaChains]) {
  switch (nc) {
    case 1: mfma_chains<1>(alds, wbl, base, koff, groups, gstride, acc); break;
    case 2: mfma_chains<2>(alds, wbl, base, koff, groups, gstride, acc); break;
    default: mfma_chains<kMfmaChains>(alds, wbl, base, koff, groups, gstride, acc); break;
  }
}

// Four waves per SIMD is what the LDS of a conv2-sized plane admits; without
// that bound the compiler spends registers on hoisted loads and halves it.
// The deep-staging bwd_data build (planes of more than 1024 cells) would
// spill under it and gets two.
//
// Forward. M = positions grouped by pool window: tile t, row r is window
// 4t + (r>>2), sub-position r&3 (row-major, the numbering of the argmax
// byte), so a lane's four accumulators are one window and ReLU, max and
// argmax stay inside the lane. N = the 16 output channels, K = CIN*9.
// LDS: [CIN][cs] halo-padded input + [K][16] weights + [tiles*16] row table.
template <int PF, bool VEC>
__global__ void __launch_bounds__(kBlock, 4) conv3x3_relu_pool_fwd_mfma_kernel(
    const float* __restrict__ in, const float* __restrict__ w, const float* __restrict__ bias,
    float* __restrict__ out, uint8_t* __restrict__ argmax, int N, int CIN, int H, int W,
    int in_vec_flag) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  constexpr int COUT = 16;
  const bool in_vec = VEC || in_vec_flag;
  const PlaneGeom pg = plane_geom(H, W);
  const int PH = H / 2, PW = W / 2;
  const int pcells = PH * PW;
  const int ocells = COUT * pcells;
  const int tiles = (pcells + 3) / 4;
  const int K = CIN * 9;
  float* ilds = (float*)smem; // [CIN][cs]
  float* wb = ilds + CIN * pg.cs; // [K][COUT]
  int* tb = (int*)(wb + K * COUT); // [tiles][16] top-left offset of a row's 3x3 stencil

  const int plane = CIN * H * W;
  const int npieces = plane / 4;

  PlaneStage<PF> st;
  st.init(npieces, H, W, pg);
  int n = blockIdx.x; // the launcher guarantees gridDim.x <= N
  st.load(in + (int64_t)n * plane, npieces, in_vec);

  for (int i = threadIdx.x; i < K * COUT; i += kBlock) wb[i] = w[(i & 15) * K + (i >> 4)];
  for (int i = threadIdx.x; i < tiles * 16; i += kBlock) {
    const int win = i >> 2, sub = i & 3;
    int base = 0; // rows past the last window read in bounds and store nothing
    if (win < pcells) {
      const int py = win / PW, px = win - py * PW;
      base = (2 * py + (sub >> 1)) * pg.PADW + 2 * px + (sub & 1);
    }
    tb[i] = base;
  }
  for (int i = threadIdx.x; i < CIN * pg.cs; i += kBlock) ilds[i] = 0.0f; // halo, once
  __syncthreads();
  st.store(in + (int64_t)n * plane, ilds, npieces, in_vec, H, W, pg);
  __syncthreads();

  const int lane = threadIdx.x & (kWave - 1);
  const int quad = lane >> 4, co = lane & 15;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x / kWave);
  const int cnt = (tiles - wave + 3) >> 2; // tiles wave, wave + 4, ... below `tiles`
  int koff[9];
#pragma unroll
  for (int s = 0; s < 9; ++s) {
    const int k = 4 * s + quad, ci = k / 9, tap = k - 9 * ci;
    koff[s] = ci * pg.cs + (tap / 3) * pg.PADW + tap % 3;
  }
  const float bz = bias[co];
  const float* wbl = wb + lane;

  for (; n < N; n += gridDim.x) {
    const int nn = n + gridDim.x;
    float* outn = out + (int64_t)n * ocells + co * pcells;
    uint8_t* argn = argmax + (int64_t)n * ocells + co * pcells;

    for (int j = 0; j < cnt; j += kMfmaChains) {
      const int nc = min(kMfmaChains, cnt - j);
      int base[kMfmaChains];
      f4 acc[kMfmaChains];
#pragma unroll
      for (int i = 0; i < kMfmaChains; ++i) {
        base[i] = tb[(wave + 4 * (j + min(i, nc - 1))) * 16 + co];
        acc[i] = f4{bz, bz, bz, bz};
      }
      mfma_tiles(nc, ilds, wbl, base, koff, CIN / 4, 4 * pg.cs, acc);

      // relu + 2x2 max of the lane's window; first index wins ties
#pragma unroll
      for (int i = 0; i < kMfmaChains; ++i) {
        const int win = 4 * (wave + 4 * (j + i)) + quad;
        if (i < nc && win < pcells) {
          const float r0 = fmaxf(acc[i].x, 0.0f);
          const float r1 = fmaxf(acc[i].y, 0.0f);
          const float r2 = fmaxf(acc[i].z, 0.0f);
          const float r3 = fmaxf(acc[i].w, 0.0f);
          float m = r0;
          int arg = 0;
          if (r1 > m) { m = r1; arg = 1; }
          if (r2 > m) { m = r2; arg = 2; }
          if (r3 > m) { m = r3; arg = 3; }
          if (!(m > 0.0f)) arg |= kGateBit;
          outn[win] = m;
          argn[win] = (uint8_t)arg;
        }
      }
    }
    __syncthreads(); // math done: ilds may be overwritten

    if (nn < N) {
      st.load(in + (int64_t)nn * plane, npieces, in_vec);
      st.store(in + (int64_t)nn * plane, ilds, npieces, in_vec, H, W, pg);
    }
    __syncthreads(); // next plane published
  }
}

// bwd_data. M = din positions in linear order y*W + x, N = the input
// channels (columns past CIN carry zero weights and are not stored),
// K = COUT*9 = 144. A lane's four accumulators are four consecutive
// positions of one channel; H*W is a multiple of 4, so they lie inside the
// channel and go out as one 16-byte store when din allows it
// (din_align: 2 = 16-byte, 1 = 8-byte, 0 = scalar stores).
// LDS: [COUT][cs] padded dconv + [K][16] weights + [tiles*16] row table.
template <int PF, bool VEC>
__global__ void __launch_bounds__(kBlock, PF == 1 ? 4 : 2) conv3x3_relu_pool_bwd_data_mfma_kernel(
    const float* __restrict__ dpooled, const uint8_t* __restrict__ argmax,
    const float* __restrict__ w, float* __restrict__ din, int N, int CIN, int H, int W,
    int cell_vec_flag, int din_align_flag) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  constexpr int COUT = 16, K = COUT * 9;
  const bool cell_vec = VEC || cell_vec_flag;
  const int din_align = VEC ? 2 : din_align_flag;
  const PlaneGeom pg = plane_geom(H, W);
  const int HW = H * W;
  const int tiles = (HW + 15) / 16;
  float* dclds = (float*)smem; // [COUT][cs]
  float* wb = dclds + COUT * pg.cs; // [K][16]
  int* tb = (int*)(wb + K * 16); // [tiles][16] padded offset of position (y, x)

  const int PH = H / 2, PW = W / 2;
  const int pcells = PH * PW;
  const int cells = COUT * pcells;

  // code = LDS offset of the top-left position of the cell's 2x2 window
  auto code_of = [&](int cell) {
    const int co = cell / pcells;
    const int rem = cell - co * pcells;
    const int py = rem / PW, px = rem - py * PW;
    return co * pg.cs + (2 * py + 1) * pg.PADW + (2 * px + 1);
  };
  auto put = [&](int code, float g, uint32_t a) {
    const float v = (a & kGateBit) ? 0.0f : g;
    const uint32_t sub = a & 3u;
    dclds[code] = (sub == 0) ? v : 0.0f;
    dclds[code + 1] = (sub == 1) ? v : 0.0f;
    dclds[code + pg.PADW] = (sub == 2) ? v : 0.0f;
    dclds[code + pg.PADW + 1] = (sub == 3) ? v : 0.0f;
  };

  CellStage<PF> st;
  st.init(cells, code_of);
  int n = blockIdx.x; // the launcher guarantees gridDim.x <= N
  st.load(dpooled + (int64_t)n * cells, argmax + (int64_t)n * cells, cells, cell_vec);

  for (int i = threadIdx.x; i < K * 16; i += kBlock) {
    const int k = i >> 4, ci = i & 15;
    const int co = k / 9, tap = k - 9 * co;
    wb[i] = (ci < CIN) ? w[(co * CIN + ci) * 9 + tap] : 0.0f;
  }
  for (int i = threadIdx.x; i < tiles * 16; i += kBlock) {
    int base = 0; // rows past the last position read in bounds and store nothing
    if (i < HW) {
      const int y = i / W;
      base = y * pg.PADW + (i - y * W);
    }
    tb[i] = base;
  }
  for (int i = threadIdx.x; i < COUT * pg.cs; i += kBlock) dclds[i] = 0.0f; // halo, once
  __syncthreads();
  st.store(dpooled + (int64_t)n * cells, argmax + (int64_t)n * cells, cells, cell_vec, code_of,
           put);
  __syncthreads();

  const int lane = threadIdx.x & (kWave - 1);
  const int quad = lane >> 4, ci = lane & 15;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x / kWave);
  const int cnt = (tiles - wave + 3) >> 2; // tiles wave, wave + 4, ... below `tiles`
  // din(y,x) += w[ky][kx] * dconv(y-ky+1, x-kx+1): padded (y-ky+2, x-kx+2)
  int koff[9];
#pragma unroll
  for (int s = 0; s < 9; ++s) {
    const int k = 4 * s + quad, co = k / 9, tap = k - 9 * co;
    koff[s] = co * pg.cs + (2 - tap / 3) * pg.PADW + (2 - tap % 3);
  }
  const float* wbl = wb + lane;

  for (; n < N; n += gridDim.x) {
    const int nn = n + gridDim.x;
    float* dinn = din + ((int64_t)n * CIN + ci) * HW;

    for (int j = 0; j < cnt; j += kMfmaChains) {
      const int nc = min(kMfmaChains, cnt - j);
      int base[kMfmaChains];
      f4 acc[kMfmaChains];
#pragma unroll
      for (int i = 0; i < kMfmaChains; ++i) {
        base[i] = tb[(wave + 4 * (j + min(i, nc - 1))) * 16 + ci];
        acc[i] = f4{0.0f, 0.0f, 0.0f, 0.0f};
      }
      mfma_tiles(nc, dclds, wbl, base, koff, COUT / 4, 4 * pg.cs, acc);

#pragma unroll
      for (int i = 0; i < kMfmaChains; ++i) {
        const int p0 = 16 * (wave + 4 * (j + i)) + 4 * quad;
        if (i < nc && p0 < HW && ci < CIN) {
          float* d = dinn + p0;
          if (din_align == 2) {
            *(f4*)d = acc[i];
          } else if (din_align == 1) {
            *(f2*)d = f2{acc[i].x, acc[i].y};
            *(f2*)(d + 2) = f2{acc[i].z, acc[i].w};
          } else {
            d[0] = acc[i].x;
            d[1] = acc[i].y;
            d[2] = acc[i].z;
            d[3] = acc[i].w;
          }
        }
      }
    }
    __syncthreads(); // math done: dclds may be overwritten
    if (nn < N) {
      st.load(dpooled + (int64_t)nn * cells, argmax + (int64_t)nn * cells, cells, cell_vec);
      st.store(dpooled + (int64_t)nn * cells, argmax + (int64_t)nn * cells, cells, cell_vec,
               code_of, put);
    }
    __syncthreads();
  }
}

// ----------------------------------------------------------- bwd weight

// End of a gather workgroup: the nslices partials of every (pair, tap) and
// of db are summed through LDS in ascending slice order (skipped when there
// is one slice), and slice 0 writes the workgroup's row of `part`. The
// caller has a barrier behind its last use of redlds' memory.
__device__ __forceinline__ void bwdw_finish_row(float (&acc)[9], float accb,
                                                float* __restrict__ redlds,
                                                float* __restrict__ part, int pairs, int nslices,
                                                int pair, int slice, int co, int ci, int COUT,
                                                bool active) {
  if (nslices > 1) {
#pragma unroll
    for (int k = 0; k < 9; ++k) {
      redlds[threadIdx.x] = active ? acc[k] : 0.0f;
      __syncthreads();
      if (active && slice == 0) {
        float total = acc[k];
        for (int sl = 1; sl < nslices; ++sl) total += redlds[sl * pairs + pair];
        acc[k] = total;
      }
      __syncthreads();
    }
    redlds[threadIdx.x] = (active && ci == 0) ? accb : 0.0f;
    __syncthreads();
    if (active && slice == 0 && ci == 0) {
      float total = accb;
      for (int sl = 1; sl < nslices; ++sl) total += redlds[sl * pairs + pair];
      accb = total;
    }
  }

  if (active && slice == 0) {
    float* row = part + (int64_t)blockIdx.x * (pairs * 9 + COUT);
#pragma unroll
    for (int k = 0; k < 9; ++k) row[pair * 9 + k] = acc[k];
    if (ci == 0) row[pairs * 9 + co] = accb;
  }
}

// Workgroup = chunk of `samples` samples looped through LDS. The pool
// gradient is pre-gated at stage time into dense per-cell (g, offset) pairs
// (g = 0 encodes "no gradient"). Thread owns ((co,ci), slice): 9 register
// partials across the chunk(s); LDS tree across slices; the workgroup
// then writes ONE row of partials {dw[pairs*9], db[COUT]} to `part`
// (row = blockIdx.x). bwd_weight_reduce_kernel sums the rows in a fixed
// order: no atomics, so the gradient does not depend on the order in which
// workgroups finish and is bitwise reproducible from run to run.
//
// The samples of a workgroup form one sequence (its chunks in ascending
// order, each chunk's samples in ascending order), staged one after the
// other: chunk boundaries need no special case.
template <int PFI, int PFC, bool VEC>
__global__ void __launch_bounds__(kBlock) conv3x3_relu_pool_bwd_weight_kernel(
    const float* __restrict__ dpooled, const uint8_t* __restrict__ argmax,
    const float* __restrict__ in, float* __restrict__ part, int N, int CIN, int COUT, int H,
    int W, int samples, int in_vec_flag, int cell_vec_flag) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const bool in_vec = VEC || in_vec_flag, cell_vec = VEC || cell_vec_flag;
  const PlaneGeom pg = plane_geom(H, W);
  const int iplane = CIN * H * W;
  const int npieces = iplane / 4;
  const int PH = H / 2, PW = W / 2;
  const int pcells = PH * PW;
  const int pstride = pooled_stride(pcells);
  float* ilds = (float*)smem; // [CIN][cs]
  float* glds = ilds + CIN * pg.cs; // [COUT][pstride] pre-gated gradients
  int* slds = (int*)(glds + COUT * pstride); // [COUT][pstride] offset of the argmax position
  float* redlds = (float*)(slds + COUT * pstride); // [kBlock]

  const int cells = COUT * pcells;

  const int pairs = COUT * CIN;
  const int nslices = max(1, kBlock / pairs);
  const int pair = threadIdx.x % pairs;
  const int slice = threadIdx.x / pairs;
  const int co = pair / CIN;
  const int ci = pair % CIN;
  const bool active = threadIdx.x < pairs * nslices;

  float acc[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
  float accb = 0.0f;

  // code = (index into glds/slds) << 16 | padded-plane offset of the top-left
  // position of the cell's window; the index is < 2^15 and the offset < 2^16
  // (LDS holds 40960 words, glds and slds half of them at most), so a code
  // is never negative
  auto code_of = [&](int cell) {
    const int cco = cell / pcells;
    const int rem = cell - cco * pcells;
    const int py = rem / PW, px = rem - py * PW;
    return ((cco * pstride + rem) << 16) | (2 * py * pg.PADW + 2 * px);
  };
  // pre-decode the argmax into a padded-plane offset so the hot loop below
  // needs no div/mod per cell
  auto put = [&](int code, float g, uint32_t a) {
    const int idx = code >> 16;
    glds[idx] = (a & kGateBit) ? 0.0f : g;
    slds[idx] = (code & 0xffff) + (int)((a >> 1) & 1u) * pg.PADW + (int)(a & 1u);
  };

  // chunk blockIdx.x and, when the grid was capped, every gridDim.x-th
  // chunk after it; all chunks of a workgroup share its accumulators
  const int nchunks = (N + samples - 1) / samples;
  int chunk = blockIdx.x; // the launcher guarantees gridDim.x <= nchunks
  int64_t n = (int64_t)chunk * samples;
  int64_t nend = min((int64_t)N, n + samples);

  PlaneStage<PFI> sti;
  CellStage<PFC> stc;
  sti.init(npieces, H, W, pg);
  stc.init(cells, code_of);
  sti.load(in + n * iplane, npieces, in_vec);
  stc.load(dpooled + n * cells, argmax + n * cells, cells, cell_vec);

  // zero the input halo ONCE; interiors are overwritten every sample
  for (int i = threadIdx.x; i < CIN * pg.cs; i += kBlock) ilds[i] = 0.0f;
  __syncthreads();
  sti.store(in + n * iplane, ilds, npieces, in_vec, H, W, pg);
  stc.store(dpooled + n * cells, argmax + n * cells, cells, cell_vec, code_of, put);
  __syncthreads();

  bool more = true;
  while (more) {
    // successor of sample n in this workgroup's sequence
    int64_t nn = n + 1;
    if (nn >= nend) {
      chunk += gridDim.x;
      nn = (int64_t)chunk * samples;
      nend = min((int64_t)N, nn + samples);
      more = chunk < nchunks;
    }
    if (active) {
      const float* ip = ilds + ci * pg.cs;
      const float* gp = glds + co * pstride;
      const int* sp = slds + co * pstride;
      for (int cell = slice; cell < pcells; cell += nslices) {
        // branchless: g == 0 cells contribute 0 to every accumulator, and
        // their stored offset still addresses in-bounds LDS — skipping
        // them would diverge the wave at 16-lane granularity
        const float g = gp[cell];
        const int off = sp[cell];
        if (ci == 0) accb += g;
        // input rows yy-1..yy+1 -> padded rows yy..yy+2, cols likewise
        const float* iw = ip + off;
#pragma unroll
        for (int ky = 0; ky < 3; ++ky) {
#pragma unroll
          for (int kx = 0; kx < 3; ++kx) {
            acc[ky * 3 + kx] = fmaf(g, iw[ky * pg.PADW + kx], acc[ky * 3 + kx]);
          }
        }
      }
    }
    __syncthreads(); // math done: the staging regions may be overwritten
    if (more) {
      sti.load(in + nn * iplane, npieces, in_vec);
      stc.load(dpooled + nn * cells, argmax + nn * cells, cells, cell_vec);
      sti.store(in + nn * iplane, ilds, npieces, in_vec, H, W, pg);
      stc.store(dpooled + nn * cells, argmax + nn * cells, cells, cell_vec, code_of, put);
    }
    __syncthreads();
    n = nn;
  }

  bwdw_finish_row(acc, accb, redlds, part, pairs, nslices, pair, slice, co, ci, COUT, active);
}

// bwd_weight as an f32 MFMA implicit GEMM, COUT == CIN == 16 only: there the
// VALU kernel above has pairs == kBlock and one slice, so every (co, ci, tap)
// is ONE serial fmaf chain over (the workgroup's sample sequence, cells in
// ascending order), and this kernel runs the same chains:
//
//   D_tap[co][ci] += sum_k A[co][k] * B_tap[k][ci],   k = 4 * cell + sub
//   A[co][k]     = pre-gated gradient of (co, cell) if sub is the argmax
//                  position, else +0.0f
//   B_tap[k][ci] = padded_in[ci][2py + (sub>>1) + ky][2px + (sub&1) + kx]
//
// One v_mfma_f32_16x16x4_f32 step is one pooled window; lane quad = lane>>4
// is the sub-position, lane&15 is co for A and ci for B, and a lane's four
// accumulators are D[4*quad .. +3][lane&15]. The dense form does 4x the
// VALU kernel's multiplications, three of four with a zero: 441 MFMAs per
// sample against 11 ds_read_b32 per 9 FMAs in the gather, which is what
// bound the VALU kernel (profiles/smallcnn_bwdw_mfma.md).
//
// Work is split over waves by tap, never by k: unit u = 0..3 owns taps u,
// u + 4, u + 8 (3/2/2/2) for the whole workgroup, as independent accumulator
// chains sharing A (rotating the three-tap unit over the waves with the
// workgroup index measured no different). db is the VALU kernel's `accb += g` chain, run by unit 1
// on the gradient it has read anyway. Chunking, the sequence of samples,
// the `part` row and the reduce kernel are those of the VALU kernel.
//
// The added zeros are fmaf(+0, x, acc), which returns acc for finite x and
// non-zero acc. Two differences from the VALU kernel remain, neither
// reachable from finite training data:
//   - a chain whose running value is -0.0 becomes +0.0 (only the sign of a
//     zero result changes);
//   - a non-finite input gives NaN at positions the sparse kernel never
//     multiplied, as torch's dense conv backward does.
//
// LDS: [16][cs] halo-padded input in a geometry of its own (no vector reads
// here, so no alignment padding: PADW = W + 2, and cs/2 odd puts the 32
// lanes of a ds_read_b32 group, 16 channels x 2 adjacent columns, on 32
// banks) + [16][ps] (gradient, sub) pairs, read as one b64 per window that
// the four quads share (ps odd: 16 channels on 16 distinct bank pairs).
// A word of B is (per-lane constant) + (wave-uniform window and tap offset):
// the sample loop has no table and no division.

__host__ __device__ __forceinline__ PlaneGeom bwdw_mfma_geom(int H, int W) {
  PlaneGeom g;
  g.PADH = H + 2;
  g.PADW = W + 2;
  g.cs = g.PADH * g.PADW; // even, as H and W are
  if ((g.cs & 2) == 0) g.cs += 2;
  return g;
}

__host__ __device__ __forceinline__ int bwdw_mfma_pstride(int pcells) { return pcells | 1; }

// One sample: the wave's NT tap chains (and the db chain) over all windows.
// The operands of window s + 1 are read before the MFMAs of window s.
template <int NT, bool DB>
__device__ __forceinline__ void bwdw_mfma_sample(const float* __restrict__ bl,
                                                 const f2* __restrict__ al, const int (&toff)[3],
                                                 int PH, int PW, int PADW, int quad,
                                                 f4 (&acc)[3], float& accb) {
  const int pcells = PH * PW;
  f2 gs = al[0];
  float b[NT];
#pragma unroll
  for (int i = 0; i < NT; ++i) b[i] = bl[toff[i]];
  int px = 0, rowoff = 0; // wave-uniform
  for (int cell = 0; cell < pcells; ++cell) {
    const f2 gs0 = gs;
    float b0[NT];
#pragma unroll
    for (int i = 0; i < NT; ++i) b0[i] = b[i];
    if (++px == PW) {
      px = 0;
      rowoff += 2 * PADW;
    }
    if (cell + 1 < pcells) {
      gs = al[cell + 1];
      const float* bp = bl + rowoff + 2 * px;
#pragma unroll
      for (int i = 0; i < NT; ++i) b[i] = bp[toff[i]];
    }
    const float a = (__float_as_int(gs0.y) == quad) ? gs0.x : 0.0f;
    if (DB) accb += gs0.x;
#pragma unroll
    for (int i = 0; i < NT; ++i) {
      acc[i] = __builtin_amdgcn_mfma_f32_16x16x4f32(a, b0[i], acc[i], 0, 0, 0);
    }
  }
}

// Four waves per SIMD, except the build that stages both operands deep
// (planes of more than 1024 cells), which would spill under that bound.
template <int PFI, int PFC, bool VEC>
__global__ void __launch_bounds__(kBlock, (PFI > 1 && PFC > 1) ? 2 : 4)
conv3x3_relu_pool_bwd_weight_mfma_kernel(
    const float* __restrict__ dpooled, const uint8_t* __restrict__ argmax,
    const float* __restrict__ in, float* __restrict__ part, int N, int H, int W, int samples,
    int in_vec_flag, int cell_vec_flag) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  constexpr int CIN = 16, COUT = 16;
  const bool in_vec = VEC || in_vec_flag, cell_vec = VEC || cell_vec_flag;
  const PlaneGeom pg = bwdw_mfma_geom(H, W);
  const int iplane = CIN * H * W;
  const int npieces = iplane / 4;
  const int PH = H / 2, PW = W / 2;
  const int pcells = PH * PW;
  const int ps = bwdw_mfma_pstride(pcells);
  float* ilds = (float*)smem; // [CIN][cs]
  f2* alds = (f2*)(ilds + CIN * pg.cs); // [COUT][ps] (pre-gated gradient, sub)
  const int cells = COUT * pcells;

  auto code_of = [&](int cell) {
    const int cco = cell / pcells;
    return cco * ps + (cell - cco * pcells);
  };
  auto put = [&](int code, float g, uint32_t a) {
    alds[code] = f2{(a & kGateBit) ? 0.0f : g, __int_as_float((int)(a & 3u))};
  };

  // chunk blockIdx.x and, when the grid was capped, every gridDim.x-th
  // chunk after it; all chunks of a workgroup share its accumulators
  const int nchunks = (N + samples - 1) / samples;
  int chunk = blockIdx.x; // the launcher guarantees gridDim.x <= nchunks
  int64_t n = (int64_t)chunk * samples;
  int64_t nend = min((int64_t)N, n + samples);

  PlaneStage<PFI> sti;
  CellStage<PFC> stc;
  sti.init(npieces, H, W, pg);
  stc.init(cells, code_of);
  sti.load(in + n * iplane, npieces, in_vec);
  stc.load(dpooled + n * cells, argmax + n * cells, cells, cell_vec);

  // zero the input halo ONCE; interiors are overwritten every sample
  for (int i = threadIdx.x; i < CIN * pg.cs; i += kBlock) ilds[i] = 0.0f;
  __syncthreads();
  sti.store(in + n * iplane, ilds, npieces, in_vec, H, W, pg);
  stc.store(dpooled + n * cells, argmax + n * cells, cells, cell_vec, code_of, put);
  __syncthreads();

  const int lane = threadIdx.x & (kWave - 1);
  const int quad = lane >> 4, col = lane & 15; // col: co of A, ci of B and D
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x / kWave);
  const int unit = wave; // one owner per accumulator, sample-invariant addresses
  int toff[3];
#pragma unroll
  for (int i = 0; i < 3; ++i) {
    const int tap = min(unit + 4 * i, 8);
    toff[i] = (tap / 3) * pg.PADW + tap % 3;
  }
  const float* bl = ilds + col * pg.cs + (quad >> 1) * pg.PADW + (quad & 1);
  const f2* al = alds + col * ps;

  f4 acc[3];
#pragma unroll
  for (int i = 0; i < 3; ++i) acc[i] = f4{0.0f, 0.0f, 0.0f, 0.0f};
  float accb = 0.0f;

  bool more = true;
  while (more) {
    // successor of sample n in this workgroup's sequence
    int64_t nn = n + 1;
    if (nn >= nend) {
      chunk += gridDim.x;
      nn = (int64_t)chunk * samples;
      nend = min((int64_t)N, nn + samples);
      more = chunk < nchunks;
    }
    if (unit == 0) {
      bwdw_mfma_sample<3, false>(bl, al, toff, PH, PW, pg.PADW, quad, acc, accb);
    } else if (unit == 1) {
      bwdw_mfma_sample<2, true>(bl, al, toff, PH, PW, pg.PADW, quad, acc, accb);
    } else {
      bwdw_mfma_sample<2, false>(bl, al, toff, PH, PW, pg.PADW, quad, acc, accb);
    }
    __syncthreads(); // math done: the staging regions may be overwritten
    if (more) {
      sti.load(in + nn * iplane, npieces, in_vec);
      stc.load(dpooled + nn * cells, argmax + nn * cells, cells, cell_vec);
      sti.store(in + nn * iplane, ilds, npieces, in_vec, H, W, pg);
      stc.store(dpooled + nn * cells, argmax + nn * cells, cells, cell_vec, code_of, put);
    }
    __syncthreads();
    n = nn;
  }

  float* row = part + (int64_t)blockIdx.x * (COUT * CIN * 9 + COUT);
#pragma unroll
  for (int i = 0; i < 3; ++i) {
    const int tap = unit + 4 * i;
    if (tap < 9) {
#pragma unroll
      for (int j = 0; j < 4; ++j) row[((4 * quad + j) * CIN + col) * 9 + tap] = acc[i][j];
    }
  }
  if (unit == 1 && quad == 0) row[COUT * CIN * 9 + col] = accb;
}

// ------------------------------------- layer-2 bwd_data + layer-1 bwd_weight
//
// The image layer needs no input gradient, so layer 2's din has one reader:
// layer 1's bwd_weight, which takes it as its dpooled. This kernel computes a
// sample's din as conv3x3_relu_pool_bwd_data_mfma_kernel does, hands it
// through LDS to the gather of conv3x3_relu_pool_bwd_weight_kernel and ends
// in that kernel's `part` row: din never goes to memory (12.5 KB per sample
// written and read back at the MNIST shapes).
//
// Notation: layer 1 is CIN1 -> C1 on H1 x W1; layer 2 is C1 -> 16 on
// H2 x W2 = H1/2 x W1/2, whose positions are layer 1's pooled cells.
//
// Bit for bit the two kernels: the MFMA phase is the bwd_data kernel's (same
// tiles, same k order; only the accumulators' destination changes), the
// gather is the VALU kernel's loop (thread = ((co, ci), slice), cells
// slice, slice + nslices, ... ascending, `accb += g`, nine fmaf in tap
// order), a workgroup's samples are the VALU kernel's sequence of chunks,
// and the cross-slice sum and the `part` row are shared code.
//
// A lane's four accumulators are four consecutive cells of channel ci. The
// gather's chain walks one cell per tile over tiles of all four waves, so
// the hand-over goes through LDS, and through dclds itself: din(n) has the
// geometry of dconv(n), which is dead once every tile of the sample is done,
// so din is written over the INTERIOR of dclds' first C1 planes. The halo
// stays zero and the next sample's staging rewrites the whole interior. A
// wave keeps its (at most kMergedHold) tile accumulators across the barrier
// behind the MFMAs; shapes with more tiles per wave are not eligible. A
// copy of its own for din would add 12.5 KB of LDS at the MNIST shapes and
// take the kernel from four workgroups per CU to three, where the
// workload's 1024 workgroups no longer fit in one round.
//
// Layer 1's argmax bytes are staged as they are and decoded in the gather:
// the gate (bit 2) selects +0.0f as the kernel above stores it, bits 0-1
// the position in the window, whose top-left offset is stepped along with
// the cell index (no division, no offset table).
//
// Sample loop:
//   A  MFMA on dclds(n); barrier; accumulators -> dclds interior. x(n) and
//      argmax1(n), loaded before the MFMAs, go to LDS behind them. barrier
//   B  gather of n; barrier; dpooled2/argmax2 of the next sample, loaded
//      before the gather, are expanded into dclds. barrier
//
// LDS: [16][cs2] padded dconv / din + [144][16] weights + [tiles*16] row
// table + [CIN1][cs1] padded x + argmax1 bytes. The cross-slice sum reuses
// the front of dclds.

typedef uint32_t u4 __attribute__((ext_vector_type(4)));
typedef int i4 __attribute__((ext_vector_type(4)));

// One sample's argmax bytes, copied to LDS unchanged. mode 2: 16-byte pieces,
// the first PF per thread loaded together ahead of their use; mode 1: 32-bit
// words; mode 0: bytes (the launcher picks by alignment and count).
template <int PF>
struct ByteStage {
  u4 v[PF];

  __device__ __forceinline__ void load(const uint8_t* __restrict__ g, int bytes, int mode) {
    if (mode != 2) return;
#pragma unroll
    for (int k = 0; k < PF; ++k) {
      const int piece = threadIdx.x + k * kBlock;
      if (16 * piece < bytes) v[k] = *(const u4*)(g + 16 * piece);
    }
  }
  __device__ __forceinline__ void store(const uint8_t* __restrict__ g, uint8_t* __restrict__ lds,
                                        int bytes, int mode) const {
    if (mode == 2) {
#pragma unroll
      for (int k = 0; k < PF; ++k) {
        const int piece = threadIdx.x + k * kBlock;
        if (16 * piece < bytes) *(u4*)(lds + 16 * piece) = v[k];
      }
      for (int piece = threadIdx.x + PF * kBlock; 16 * piece < bytes; piece += kBlock) {
        *(u4*)(lds + 16 * piece) = *(const u4*)(g + 16 * piece);
      }
    } else if (mode == 1) {
      for (int i = threadIdx.x; 4 * i < bytes; i += kBlock) {
        ((uint32_t*)lds)[i] = ((const uint32_t*)g)[i];
      }
    } else {
      for (int i = threadIdx.x; i < bytes; i += kBlock) lds[i] = g[i];
    }
  }
};

constexpr int kMergedHold = kMfmaChains + 1; // tiles per wave kept in registers

// The value, made opaque to the optimizer. The merged kernel runs at the
// register limit of four waves per SIMD: what is derived from an opaque
// value inside the sample loop (per-thread 64-bit load addresses) or behind
// it (the roles of the final reduction) is worked out there, in a few
// instructions, and holds no register across the MFMA phase.
__device__ __forceinline__ int opaque(int v) {
  asm volatile("" : "+v"(v));
  return v;
}

// Four waves per SIMD is what the LDS admits at the MNIST shapes. The build
// that stages x deep and the builds for unaligned bases would spill under
// that bound and get two. Layer 2's cells and the argmax1 bytes are at most
// one 16-byte piece per thread: eligible shapes have
// H2 * W2 <= 16 * kMergedHold = kBlock positions.
template <int PFX, bool VEC>
__global__ void __launch_bounds__(kBlock, (PFX > 1 || !VEC) ? 2 : 4)
conv3x3_relu_pool_bwd_data_weight_kernel(
    const float* __restrict__ dpooled2, const uint8_t* __restrict__ argmax2,
    const float* __restrict__ w2, const uint8_t* __restrict__ argmax1,
    const float* __restrict__ x, float* __restrict__ part, int N, int CIN1, int C1, int H1,
    int W1, int samples, int x_vec_flag, int cell_vec_flag, int am1_mode_flag) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  constexpr int COUT2 = 16, K = COUT2 * 9;
  const bool x_vec = VEC || x_vec_flag, cell_vec = VEC || cell_vec_flag;
  const int am1_mode = VEC ? 2 : am1_mode_flag;
  const int H2 = H1 / 2, W2 = W1 / 2;
  const PlaneGeom pg1 = plane_geom(H1, W1), pg2 = plane_geom(H2, W2);
  const int HW2 = H2 * W2; // layer 2 positions = layer 1 pooled cells
  const int tiles = (HW2 + 15) / 16;
  const int xplane = CIN1 * H1 * W1;
  const int xpieces = xplane / 4;
  const int cells1 = C1 * HW2;
  const int PH2 = H2 / 2, PW2 = W2 / 2;
  const int pcells2 = PH2 * PW2;
  const int cells2 = COUT2 * pcells2;

  float* dclds = (float*)smem; // [COUT2][cs2]
  float* wb = dclds + COUT2 * pg2.cs; // [K][16]
  int* tb = (int*)(wb + K * 16); // [tiles][16] padded offset of position (y, x)
  float* ilds = (float*)(tb + tiles * 16); // [CIN1][cs1]
  uint8_t* alds = (uint8_t*)(ilds + CIN1 * pg1.cs); // [C1][HW2] argmax1 bytes
  float* redlds = dclds; // [kBlock], after the sample loop

  // layer 2 staging: as in conv3x3_relu_pool_bwd_data_mfma_kernel
  auto code_of = [&](int cell) {
    const int co = cell / pcells2;
    const int rem = cell - co * pcells2;
    const int py = rem / PW2, px = rem - py * PW2;
    return co * pg2.cs + (2 * py + 1) * pg2.PADW + (2 * px + 1);
  };
  auto put = [&](int code, float g, uint32_t a) {
    const float v = (a & kGateBit) ? 0.0f : g;
    const uint32_t sub = a & 3u;
    float* d = dclds + opaque(code); // the second row's address is not kept either
    d[0] = (sub == 0) ? v : 0.0f;
    d[1] = (sub == 1) ? v : 0.0f;
    d[pg2.PADW] = (sub == 2) ? v : 0.0f;
    d[pg2.PADW + 1] = (sub == 3) ? v : 0.0f;
  };

  // chunk blockIdx.x and, when the grid was capped, every gridDim.x-th
  // chunk after it; all chunks of a workgroup share its accumulators
  const int nchunks = (N + samples - 1) / samples;
  int chunk = blockIdx.x; // the launcher guarantees gridDim.x <= nchunks
  int64_t n = (int64_t)chunk * samples;
  int64_t nend = min((int64_t)N, n + samples);

  // eligible shapes: one piece per thread covers layer 2's cells and the
  // argmax1 bytes (and x when PFX == 1), so the stagers' tail loops are dead
  __builtin_assume(cells2 <= 4 * kBlock);
  __builtin_assume(cells1 <= 16 * kBlock);
  __builtin_assume(PFX > 1 || xpieces <= kBlock);
  PlaneStage<PFX> sx;
  CellStage<1> sc;
  ByteStage<1> sa;
  sx.init(xpieces, H1, W1, pg1);
  sc.init(cells2, code_of);
  sc.load(dpooled2 + n * cells2, argmax2 + n * cells2, cells2, cell_vec);

  for (int i = threadIdx.x; i < K * 16; i += kBlock) {
    const int k = i >> 4, c = i & 15;
    const int co = k / 9, tap = k - 9 * co;
    wb[i] = (c < C1) ? w2[(co * C1 + c) * 9 + tap] : 0.0f;
  }
  for (int i = threadIdx.x; i < tiles * 16; i += kBlock) {
    int base = 0; // rows past the last position read in bounds and store nothing
    if (i < HW2) {
      const int y = i / W2;
      base = y * pg2.PADW + (i - y * W2);
    }
    tb[i] = base;
  }
  // halos, once: interiors are overwritten every sample
  for (int i = threadIdx.x; i < COUT2 * pg2.cs; i += kBlock) dclds[i] = 0.0f;
  for (int i = threadIdx.x; i < CIN1 * pg1.cs; i += kBlock) ilds[i] = 0.0f;
  __syncthreads();
  sc.store(dpooled2 + n * cells2, argmax2 + n * cells2, cells2, cell_vec, code_of, put);
  __syncthreads();

  // MFMA phase roles
  const int lane = threadIdx.x & (kWave - 1);
  const int quad = lane >> 4, mc = lane & 15; // mc: din channel of the lane
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x / kWave);
  const int cnt = (tiles - wave + 3) >> 2; // tiles wave, wave + 4, ... below `tiles`
  int koff[9];
#pragma unroll
  for (int s = 0; s < 9; ++s) {
    const int k = 4 * s + quad, co = k / 9, tap = k - 9 * co;
    koff[s] = co * pg2.cs + (2 - tap / 3) * pg2.PADW + (2 - tap % 3);
  }
  const float* wbl = wb + lane;
  // din(y, x) of channel c lies where dconv(y, x) of channel c did
  float* gl = dclds + mc * pg2.cs + pg2.PADW + 1;
  // tile `wave + 4 * j`: four positions of channel mc (they may span two
  // rows, so four stores)
  auto emit = [&](int j, const f4& a) {
    const int r0 = 16 * (wave + 4 * j) + 4 * quad;
    if (r0 < HW2 && mc < C1) { // HW2 % 4 == 0: r0 + 3 < HW2 too
      const i4 o = *(const i4*)(tb + r0);
      gl[o.x] = a.x;
      gl[o.y] = a.y;
      gl[o.z] = a.z;
      gl[o.w] = a.w;
    }
  };

  // gather phase roles
  const int pairs = C1 * CIN1;
  const int nslices = max(1, kBlock / pairs);
  const int pair = threadIdx.x % pairs;
  const int slice = threadIdx.x / pairs;
  const int co = pair / CIN1;
  const int ci = pair % CIN1;
  const bool active = threadIdx.x < pairs * nslices;
  // top-left padded offset of the window of cell `slice`, and its step to
  // cell + nslices: W2 cells per row, two padded rows and columns per cell
  const int pyx0 = (slice / W2) << 16 | (slice % W2); // cell `slice`: (py, px) in one register
  const int pxstep = nslices % W2;
  const int offstep = 2 * (nslices / W2) * pg1.PADW + 2 * pxstep;
  const int offwrap = 2 * pg1.PADW - 2 * W2;
  // the same walk over din in dclds
  const int goffstep = (nslices / W2) * pg2.PADW + pxstep;
  const int goffwrap = pg2.PADW - W2;

  float acc[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
  float accb = 0.0f;

  while (true) {
    // successor of sample n in this workgroup's sequence
    bool more = true;
    int64_t nn = n + 1;
    if (nn >= nend) {
      chunk += gridDim.x;
      nn = (int64_t)chunk * samples;
      nend = min((int64_t)N, nn + samples);
      more = chunk < nchunks;
    }

    // ---- A: din of sample n over dconv(n)
    const int z = opaque(0);
    const float* xn = x + n * xplane + z;
    const uint8_t* a1n = argmax1 + n * cells1 + z;
    sx.load(xn, xpieces, x_vec);
    sa.load(a1n, cells1, am1_mode);
    {
      // cnt <= kMergedHold: chains of three tiles, then the fourth
      int base[kMfmaChains];
      f4 a0[kMfmaChains], a1[kMfmaChains]; // of a1 only [0] is live
      const int nc = min(kMfmaChains, cnt); // 0 for a wave past the last tile
#pragma unroll
      for (int i = 0; i < kMfmaChains; ++i) {
        base[i] = tb[min(wave + 4 * max(0, min(i, nc - 1)), tiles - 1) * 16 + mc];
        a0[i] = f4{0.0f, 0.0f, 0.0f, 0.0f};
      }
      if (nc > 0) mfma_tiles(nc, dclds, wbl, base, koff, COUT2 / 4, 4 * pg2.cs, a0);
      a1[0] = f4{0.0f, 0.0f, 0.0f, 0.0f};
      if (cnt > kMfmaChains) {
        base[0] = tb[(wave + 4 * kMfmaChains) * 16 + mc];
        mfma_chains<1>(dclds, wbl, base, koff, COUT2 / 4, 4 * pg2.cs, a1);
      }
      __syncthreads(); // every wave is done reading dconv(n)
#pragma unroll
      for (int i = 0; i < kMfmaChains; ++i) {
        if (i < nc) emit(i, a0[i]);
      }
      if (cnt > kMfmaChains) emit(kMfmaChains, a1[0]);
    }
    sx.store(xn, ilds, xpieces, x_vec, H1, W1, pg1);
    sa.store(a1n, alds, cells1, am1_mode);
    __syncthreads();

    // ---- B: gather of sample n
    const float* dpn = dpooled2 + nn * cells2 + z;
    const uint8_t* a2n = argmax2 + nn * cells2 + z;
    if (more) sc.load(dpn, a2n, cells2, cell_vec);
    if (active) {
      const float* ip = ilds + ci * pg1.cs;
      const float* gp = dclds + co * pg2.cs + pg2.PADW + 1;
      const uint8_t* ap = alds + co * HW2;
      const int pyx = opaque(pyx0), py0 = pyx >> 16;
      int px = pyx & 0xffff;
      int off = 2 * py0 * pg1.PADW + 2 * px, goff = py0 * pg2.PADW + px;
      for (int cell = slice; cell < HW2; cell += nslices) {
        // branchless, as in conv3x3_relu_pool_bwd_weight_kernel: a gated
        // cell contributes g = +0.0f through an in-bounds window
        const uint32_t a = ap[cell];
        const float gv = gp[goff];
        const float g = (a & kGateBit) ? 0.0f : gv;
        if (ci == 0) accb += g;
        const float* iw = ip + off + (int)((a >> 1) & 1u) * pg1.PADW + (int)(a & 1u);
#pragma unroll
        for (int ky = 0; ky < 3; ++ky) {
#pragma unroll
          for (int kx = 0; kx < 3; ++kx) {
            acc[ky * 3 + kx] = fmaf(g, iw[ky * pg1.PADW + kx], acc[ky * 3 + kx]);
          }
        }
        px += pxstep;
        off += offstep;
        goff += goffstep;
        if (px >= W2) {
          px -= W2;
          off += offwrap;
          goff += goffwrap;
        }
      }
    }
    __syncthreads(); // din(n) read: dclds may be refilled
    if (more) sc.store(dpn, a2n, cells2, cell_vec, code_of, put);
    __syncthreads();
    if (!more) break;
    n = nn;
  }

  const int t = opaque((int)threadIdx.x), fpairs = opaque(pairs); // the gather's roles again
  const int fpair = t % fpairs, fslice = t / fpairs;
  bwdw_finish_row(acc, accb, redlds, part, pairs, nslices, fpair, fslice, fpair / CIN1,
                  fpair % CIN1, C1, t < pairs * nslices);
}

// Sums the `rows` partial rows of `part` [rows][cols] column by column in a
// fixed order and STORES the totals to dw (cols < ndw) / db (the rest; may
// be null), which need not be initialised. Workgroup = kRedCols columns x
// kRedGroups row groups: a thread sums rows g, g + kRedGroups, ... of its
// column, then group 0 combines the kRedGroups partials through LDS in
// ascending order.
constexpr int kRedCols = 16;
constexpr int kRedGroups = kBlock / kRedCols;
__global__ void __launch_bounds__(kBlock) bwd_weight_reduce_kernel(
    const float* __restrict__ part, float* __restrict__ dw, float* __restrict__ db, int rows,
    int cols, int ndw) {
  __shared__ float red[kRedGroups][kRedCols + 1];
  const int c = threadIdx.x % kRedCols;
  const int g = threadIdx.x / kRedCols;
  const int col = blockIdx.x * kRedCols + c;
  float total = 0.0f;
  if (col < cols) {
#pragma unroll 8
    for (int r = g; r < rows; r += kRedGroups) total += part[(int64_t)r * cols + col];
  }
  red[g][c] = total;
  __syncthreads();
  if (g == 0 && col < cols) {
    for (int j = 1; j < kRedGroups; ++j) total += red[j][c];
    if (col < ndw) {
      dw[col] = total;
    } else if (db != nullptr) {
      db[col - ndw] = total;
    }
  }
}

// ------------------------------------------------------------ launchers

static constexpr int kMaxLds = 160 * 1024;

static bool aligned_to(const void* p, uintptr_t bytes) { return ((uintptr_t)p % bytes) == 0; }

// dpooled as float4 and argmax as 32-bit words: every sample must start on
// such a boundary
static bool cells_vectorizable(const at::Tensor& dpooled, const at::Tensor& argmax, int cells) {
  return cells % 4 == 0 && aligned_to(dpooled.data_ptr(), 16) && aligned_to(argmax.data_ptr(), 4);
}

// staging registers per thread: 1 when one float4 piece per thread covers
// the sample (the MNIST shapes' smaller operand), else 4 (the larger one);
// what 4 * kBlock pieces do not cover is copied piece by piece
static int stage_depth(int pieces) { return pieces <= kBlock ? 1 : 4; }

// Shapes that forward and bwd_data run as an f32 MFMA implicit GEMM
// (bwd_weight: CIN == 16 among them only).
// DMLCLOUD_SMALLCNN_MFMA=0 (read per call) forces the VALU kernels.
static bool mfma_eligible(int CIN, int COUT) {
  if (COUT != 16 || CIN % 4 != 0 || CIN > 16) return false;
  const char* env = std::getenv("DMLCLOUD_SMALLCNN_MFMA");
  return env == nullptr || atoi(env) != 0;
}

// Samples per chunk of the bwd_weight kernels: chunk so that the grid stays
// ~>= 512 blocks while cutting partial rows
// (DMLCLOUD_SMALLCNN_BWDW_CHUNK overrides for tuning experiments)
static int bwdw_chunk_samples(int N) {
  if (const char* env = std::getenv("DMLCLOUD_SMALLCNN_BWDW_CHUNK")) {
    return std::max(1, atoi(env));
  }
  int samples = 1;
  while (samples < 16 && (N + samples * 2 - 1) / (samples * 2) >= 512) samples *= 2;
  return samples;
}

void conv3x3_relu_pool_fwd(at::Tensor in, at::Tensor w, at::Tensor b, at::Tensor out,
                           at::Tensor argmax) {
  TORCH_CHECK(in.is_cuda() && in.scalar_type() == at::kFloat && in.is_contiguous(),
              "input must be contiguous fp32 on device");
  TORCH_CHECK(w.is_contiguous() && b.is_contiguous(), "weights must be contiguous");
  TORCH_CHECK(w.size(2) == 3 && w.size(3) == 3, "kernel must be 3x3");
  const int N = in.size(0), CIN = in.size(1), H = in.size(2), W = in.size(3);
  const int COUT = w.size(0);
  TORCH_CHECK(H % 2 == 0 && W % 2 == 0, "H and W must be even for 2x2 pooling");
  TORCH_CHECK(w.size(1) == CIN, "weight in-channels must match input");
  TORCH_CHECK(b.numel() == COUT, "bias must be [COUT]");
  TORCH_CHECK(out.numel() == (int64_t)N * COUT * (H / 2) * (W / 2) && out.is_contiguous(),
              "out must be contiguous [N,COUT,H/2,W/2]");
  TORCH_CHECK(argmax.numel() == out.numel() && argmax.scalar_type() == at::kByte &&
                  argmax.is_contiguous(),
              "argmax must be contiguous uint8 like out");
  const PlaneGeom pg = plane_geom(H, W);
  const int lds_bytes = (CIN * pg.cs + COUT * CIN * 9 + COUT) * (int)sizeof(float);
  TORCH_CHECK(lds_bytes <= kMaxLds, "plane+weights exceed LDS (", lds_bytes, " B)");
  if (N == 0) return;
  auto stream = c10::hip::getCurrentHIPStream();
  const int blocks = std::min(N, kMaxGrid);
  const int in_vec = aligned_to(in.data_ptr(), 16);
  const bool deep = stage_depth(CIN * H * W / 4) > 1;
  const int gemm_tiles = ((H / 2) * (W / 2) + 3) / 4;
  const int mfma_lds = (CIN * pg.cs + COUT * CIN * 9 + gemm_tiles * 16) * (int)sizeof(float);
  if (mfma_eligible(CIN, COUT) && mfma_lds <= kMaxLds) {
    auto kernel = in_vec ? (deep ? conv3x3_relu_pool_fwd_mfma_kernel<4, true>
                                 : conv3x3_relu_pool_fwd_mfma_kernel<1, true>)
                         : (deep ? conv3x3_relu_pool_fwd_mfma_kernel<4, false>
                                 : conv3x3_relu_pool_fwd_mfma_kernel<1, false>);
    hipLaunchKernelGGL(kernel, dim3(blocks), dim3(kBlock), mfma_lds, stream,
                       in.data_ptr<float>(), w.data_ptr<float>(), b.data_ptr<float>(),
                       out.data_ptr<float>(), argmax.data_ptr<uint8_t>(), N, CIN, H, W, in_vec);
    return;
  }
  auto kernel = in_vec ? (deep ? conv3x3_relu_pool_fwd_kernel<4, true>
                               : conv3x3_relu_pool_fwd_kernel<1, true>)
                       : (deep ? conv3x3_relu_pool_fwd_kernel<4, false>
                               : conv3x3_relu_pool_fwd_kernel<1, false>);
  hipLaunchKernelGGL(kernel, dim3(blocks), dim3(kBlock), lds_bytes, stream,
                     in.data_ptr<float>(), w.data_ptr<float>(), b.data_ptr<float>(),
                     out.data_ptr<float>(), argmax.data_ptr<uint8_t>(), N, CIN, COUT, H, W,
                     in_vec);
}

void conv3x3_relu_pool_bwd_data(at::Tensor dpooled, at::Tensor argmax, at::Tensor w,
                                at::Tensor din) {
  const int N = din.size(0), CIN = din.size(1), H = din.size(2), W = din.size(3);
  const int COUT = w.size(0);
  TORCH_CHECK(w.size(1) == CIN && din.is_contiguous(), "weight/din geometry mismatch");
  TORCH_CHECK(dpooled.numel() == (int64_t)N * COUT * (H / 2) * (W / 2) &&
                  argmax.numel() == dpooled.numel() && dpooled.is_contiguous() &&
                  argmax.is_contiguous(),
              "dpooled/argmax must be contiguous [N,COUT,H/2,W/2]");
  const PlaneGeom pg = plane_geom(H, W);
  const int lds_bytes = (COUT * pg.cs + COUT * CIN * 9) * (int)sizeof(float);
  TORCH_CHECK(lds_bytes <= kMaxLds, "dconv plane exceeds LDS");
  if (N == 0) return;
  auto stream = c10::hip::getCurrentHIPStream();
  const int blocks = std::min(N, kMaxGrid);
  const int cells = COUT * (H / 2) * (W / 2);
  const int cell_vec = cells_vectorizable(dpooled, argmax, cells);
  const int din_vec = aligned_to(din.data_ptr(), 8);
  const bool deep = stage_depth((cells + 3) / 4) > 1;
  const int gemm_tiles = (H * W + 15) / 16;
  const int mfma_lds = (COUT * pg.cs + COUT * 9 * 16 + gemm_tiles * 16) * (int)sizeof(float);
  if (mfma_eligible(CIN, COUT) && mfma_lds <= kMaxLds) {
    const int din_align = aligned_to(din.data_ptr(), 16) ? 2 : din_vec;
    auto kernel = (cell_vec && din_align == 2)
                      ? (deep ? conv3x3_relu_pool_bwd_data_mfma_kernel<4, true>
                              : conv3x3_relu_pool_bwd_data_mfma_kernel<1, true>)
                      : (deep ? conv3x3_relu_pool_bwd_data_mfma_kernel<4, false>
                              : conv3x3_relu_pool_bwd_data_mfma_kernel<1, false>);
    hipLaunchKernelGGL(kernel, dim3(blocks), dim3(kBlock), mfma_lds, stream,
                       dpooled.data_ptr<float>(), argmax.data_ptr<uint8_t>(), w.data_ptr<float>(),
                       din.data_ptr<float>(), N, CIN, H, W, cell_vec, din_align);
    return;
  }
  auto kernel = (cell_vec && din_vec) ? (deep ? conv3x3_relu_pool_bwd_data_kernel<4, true>
                                              : conv3x3_relu_pool_bwd_data_kernel<1, true>)
                                      : (deep ? conv3x3_relu_pool_bwd_data_kernel<4, false>
                                              : conv3x3_relu_pool_bwd_data_kernel<1, false>);
  hipLaunchKernelGGL(kernel, dim3(blocks), dim3(kBlock), lds_bytes, stream,
                     dpooled.data_ptr<float>(), argmax.data_ptr<uint8_t>(), w.data_ptr<float>(),
                     din.data_ptr<float>(), N, CIN, COUT, H, W, cell_vec, din_vec);
}

void conv3x3_relu_pool_bwd_weight(at::Tensor dpooled, at::Tensor argmax, at::Tensor in,
                                  at::Tensor dw, at::Tensor db) {
  const int N = in.size(0), CIN = in.size(1), H = in.size(2), W = in.size(3);
  const int COUT = dw.size(0);
  TORCH_CHECK(COUT * CIN <= kBlock, "bwd_weight supports COUT*CIN <= ", kBlock);
  TORCH_CHECK(in.is_contiguous() && dpooled.is_contiguous() && argmax.is_contiguous(),
              "in/dpooled/argmax must be contiguous");
  const PlaneGeom pg = plane_geom(H, W);
  const int pcells = (H / 2) * (W / 2);
  const int pstride = pooled_stride(pcells);
  const int lds_bytes =
      (CIN * pg.cs + 2 * COUT * pstride + kBlock) * (int)sizeof(float);
  TORCH_CHECK(lds_bytes <= kMaxLds, "bwd_weight staging exceeds LDS (", lds_bytes, " B)");
  TORCH_CHECK(dw.is_contiguous() && dw.scalar_type() == at::kFloat &&
                  dw.numel() == (int64_t)COUT * CIN * 9,
              "dw must be contiguous fp32 [COUT,CIN,3,3]");
  TORCH_CHECK(!db.defined() || (db.is_contiguous() && db.numel() == COUT), "db must be [COUT]");
  const int samples = bwdw_chunk_samples(N);
  if (N == 0) { // nothing to sum: the gradient of an empty batch is zero
    dw.zero_();
    if (db.defined()) db.zero_();
    return;
  }
  // one partial row per workgroup; the grid cap bounds the workspace
  const int blocks = std::min((N + samples - 1) / samples, kMaxGrid);
  const int ndw = COUT * CIN * 9;
  const int cols = ndw + COUT;
  at::Tensor part = at::empty({blocks, cols}, dw.options());
  auto stream = c10::hip::getCurrentHIPStream();
  const int cells = COUT * pcells;
  const int in_vec = aligned_to(in.data_ptr(), 16);
  const int cell_vec = cells_vectorizable(dpooled, argmax, cells);
  const int pfi = stage_depth(CIN * H * W / 4), pfc = stage_depth((cells + 3) / 4);
  // COUT == CIN == 16 is the one shape whose VALU chains are whole per
  // (co, ci, tap), which the MFMA form reproduces bit for bit
  const int mfma_lds = (CIN * bwdw_mfma_geom(H, W).cs + 2 * COUT * bwdw_mfma_pstride(pcells)) *
                       (int)sizeof(float);
  if (CIN == 16 && mfma_eligible(CIN, COUT) && mfma_lds <= kMaxLds) {
    auto mkernel =
        (in_vec && cell_vec)
            ? (pfi == 1 ? (pfc == 1 ? conv3x3_relu_pool_bwd_weight_mfma_kernel<1, 1, true>
                                    : conv3x3_relu_pool_bwd_weight_mfma_kernel<1, 4, true>)
                        : (pfc == 1 ? conv3x3_relu_pool_bwd_weight_mfma_kernel<4, 1, true>
                                    : conv3x3_relu_pool_bwd_weight_mfma_kernel<4, 4, true>))
            : (pfi == 1 ? (pfc == 1 ? conv3x3_relu_pool_bwd_weight_mfma_kernel<1, 1, false>
                                    : conv3x3_relu_pool_bwd_weight_mfma_kernel<1, 4, false>)
                        : (pfc == 1 ? conv3x3_relu_pool_bwd_weight_mfma_kernel<4, 1, false>
                                    : conv3x3_relu_pool_bwd_weight_mfma_kernel<4, 4, false>));
    hipLaunchKernelGGL(mkernel, dim3(blocks), dim3(kBlock), mfma_lds, stream,
                       dpooled.data_ptr<float>(), argmax.data_ptr<uint8_t>(),
                       in.data_ptr<float>(), part.data_ptr<float>(), N, H, W, samples, in_vec,
                       cell_vec);
    hipLaunchKernelGGL(bwd_weight_reduce_kernel, dim3((cols + kRedCols - 1) / kRedCols),
                       dim3(kBlock), 0, stream, part.data_ptr<float>(), dw.data_ptr<float>(),
                       db.defined() ? db.data_ptr<float>() : nullptr, blocks, cols, ndw);
    return;
  }
  auto kernel =
      (in_vec && cell_vec)
          ? (pfi == 1 ? (pfc == 1 ? conv3x3_relu_pool_bwd_weight_kernel<1, 1, true>
                                  : conv3x3_relu_pool_bwd_weight_kernel<1, 4, true>)
                      : (pfc == 1 ? conv3x3_relu_pool_bwd_weight_kernel<4, 1, true>
                                  : conv3x3_relu_pool_bwd_weight_kernel<4, 4, true>))
          : (pfi == 1 ? (pfc == 1 ? conv3x3_relu_pool_bwd_weight_kernel<1, 1, false>
                                  : conv3x3_relu_pool_bwd_weight_kernel<1, 4, false>)
                      : (pfc == 1 ? conv3x3_relu_pool_bwd_weight_kernel<4, 1, false>
                                  : conv3x3_relu_pool_bwd_weight_kernel<4, 4, false>));
  hipLaunchKernelGGL(kernel, dim3(blocks), dim3(kBlock), lds_bytes, stream,
                     dpooled.data_ptr<float>(), argmax.data_ptr<uint8_t>(), in.data_ptr<float>(),
                     part.data_ptr<float>(), N, CIN, COUT, H, W, samples, in_vec, cell_vec);
  hipLaunchKernelGGL(bwd_weight_reduce_kernel, dim3((cols + kRedCols - 1) / kRedCols),
                     dim3(kBlock), 0, stream, part.data_ptr<float>(), dw.data_ptr<float>(),
                     db.defined() ? db.data_ptr<float>() : nullptr, blocks, cols, ndw);
}

// Layer 2's bwd_data and layer 1's bwd_weight of the two-layer stack
//   x [N,CIN1,H1,W1] -> layer 1 (C1 channels) -> layer 2 (16 channels),
// for a layer 1 that needs no input gradient: dw1/db1 from layer 2's pool
// gradient. Eligible shapes run conv3x3_relu_pool_bwd_data_weight_kernel;
// the others, and every shape with DMLCLOUD_SMALLCNN_MERGE_BWD=0 (read per
// call), run the two launchers above on a temporary din. Both give the same
// bits.
void conv3x3_relu_pool_bwd_data_weight(at::Tensor dpooled2, at::Tensor argmax2, at::Tensor w2,
                                       at::Tensor argmax1, at::Tensor x, at::Tensor dw1,
                                       at::Tensor db1) {
  auto dev_ok = [&](const at::Tensor& t, at::ScalarType st) {
    return t.defined() && t.is_cuda() && t.device() == x.device() && t.scalar_type() == st &&
           t.is_contiguous();
  };
  TORCH_CHECK(x.defined() && x.is_cuda() && x.dim() == 4, "x must be a 4-d device tensor");
  TORCH_CHECK(dev_ok(x, at::kFloat), "x must be contiguous fp32 on device");
  TORCH_CHECK(dev_ok(dpooled2, at::kFloat), "dpooled2 must be contiguous fp32 on x's device");
  TORCH_CHECK(dev_ok(w2, at::kFloat), "w2 must be contiguous fp32 on x's device");
  TORCH_CHECK(dev_ok(dw1, at::kFloat), "dw1 must be contiguous fp32 on x's device");
  TORCH_CHECK(dev_ok(db1, at::kFloat), "db1 must be contiguous fp32 on x's device");
  TORCH_CHECK(dev_ok(argmax1, at::kByte), "argmax1 must be contiguous uint8 on x's device");
  TORCH_CHECK(dev_ok(argmax2, at::kByte), "argmax2 must be contiguous uint8 on x's device");
  const int64_t N = x.size(0), CIN1 = x.size(1), H1 = x.size(2), W1 = x.size(3);
  TORCH_CHECK(dw1.dim() == 4 && dw1.size(1) == CIN1 && dw1.size(2) == 3 && dw1.size(3) == 3,
              "dw1 must be [C1,CIN1,3,3]");
  const int64_t C1 = dw1.size(0);
  TORCH_CHECK(w2.dim() == 4 && w2.size(1) == C1 && w2.size(2) == 3 && w2.size(3) == 3,
              "w2 must be [C2,C1,3,3]");
  const int64_t C2 = w2.size(0);
  // both layers pool 2x2
  TORCH_CHECK(H1 > 0 && W1 > 0 && H1 % 4 == 0 && W1 % 4 == 0,
              "H1 and W1 must be multiples of 4 for two 2x2 poolings");
  const int64_t H2 = H1 / 2, W2 = W1 / 2;
  TORCH_CHECK(db1.numel() == C1, "db1 must be [C1]");
  TORCH_CHECK(argmax1.sizes() == at::IntArrayRef({N, C1, H2, W2}),
              "argmax1 must be [N,C1,H1/2,W1/2]");
  TORCH_CHECK(dpooled2.sizes() == at::IntArrayRef({N, C2, H2 / 2, W2 / 2}),
              "dpooled2 must be [N,C2,H1/4,W1/4]");
  TORCH_CHECK(argmax2.sizes() == dpooled2.sizes(), "argmax2 must be shaped like dpooled2");
  TORCH_CHECK(C1 * CIN1 <= kBlock, "bwd_weight supports COUT*CIN <= ", kBlock);

  const PlaneGeom pg1 = plane_geom(H1, W1), pg2 = plane_geom(H2, W2);
  const int64_t HW2 = H2 * W2;
  const int64_t tiles = (HW2 + 15) / 16;
  const int64_t cells1 = C1 * HW2;
  const int64_t lds_bytes =
      (16 * pg2.cs + 16 * 9 * 16 + tiles * 16 + CIN1 * pg1.cs) * (int64_t)sizeof(float) +
      ((cells1 + 15) & ~(int64_t)15);
  const char* env = std::getenv("DMLCLOUD_SMALLCNN_MERGE_BWD");
  const bool merged = (env == nullptr || atoi(env) != 0) && mfma_eligible(C1, C2) &&
                      tiles <= 4 * kMergedHold && lds_bytes <= kMaxLds;
  if (!merged) {
    at::Tensor din = at::empty({N, C1, H2, W2}, x.options());
    conv3x3_relu_pool_bwd_data(dpooled2, argmax2, w2, din);
    conv3x3_relu_pool_bwd_weight(din, argmax1, x, dw1, db1);
    return;
  }
  if (N == 0) { // nothing to sum: the gradient of an empty batch is zero
    dw1.zero_();
    db1.zero_();
    return;
  }
  const int samples = bwdw_chunk_samples(N);
  const int blocks = std::min(((int)N + samples - 1) / samples, kMaxGrid);
  const int ndw = C1 * CIN1 * 9;
  const int cols = ndw + C1;
  at::Tensor part = at::empty({blocks, cols}, dw1.options());
  auto stream = c10::hip::getCurrentHIPStream();
  const int cells2 = 16 * (H2 / 2) * (W2 / 2);
  const int x_vec = aligned_to(x.data_ptr(), 16);
  const int cell_vec = cells_vectorizable(dpooled2, argmax2, cells2);
  const int am1_mode = (cells1 % 16 == 0 && aligned_to(argmax1.data_ptr(), 16)) ? 2
                       : aligned_to(argmax1.data_ptr(), 4)                       ? 1
                                                                                 : 0;
  const bool deep = stage_depth(CIN1 * H1 * W1 / 4) > 1;
  auto kernel = (x_vec && cell_vec && am1_mode == 2)
                    ? (deep ? conv3x3_relu_pool_bwd_data_weight_kernel<4, true>
                            : conv3x3_relu_pool_bwd_data_weight_kernel<1, true>)
                    : (deep ? conv3x3_relu_pool_bwd_data_weight_kernel<4, false>
                            : conv3x3_relu_pool_bwd_data_weight_kernel<1, false>);
  hipLaunchKernelGGL(kernel, dim3(blocks), dim3(kBlock), (int)lds_bytes, stream,
                     dpooled2.data_ptr<float>(), argmax2.data_ptr<uint8_t>(),
                     w2.data_ptr<float>(), argmax1.data_ptr<uint8_t>(), x.data_ptr<float>(),
                     part.data_ptr<float>(), (int)N, (int)CIN1, (int)C1, (int)H1, (int)W1,
                     samples, x_vec, cell_vec, am1_mode);
  hipLaunchKernelGGL(bwd_weight_reduce_kernel, dim3((cols + kRedCols - 1) / kRedCols),
                     dim3(kBlock), 0, stream, part.data_ptr<float>(), dw1.data_ptr<float>(),
                     db1.data_ptr<float>(), blocks, cols, ndw);
}

} // namespace dmlamd
