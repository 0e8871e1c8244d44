// kvcache_append: write the K and V rows of Nq new tokens per batch row into a
// K/V cache, dense or paged, at the positions sdpa_kvcache gives the same
// query rows (ops.fused_attn.kvcache_append). Part of attention.hip (included
// at its end, inside namespace dmlamd); it uses that file's Strides,
// decode_len, check_block_table and NamedTensor.
//
// Contract. k_new, v_new [B, Hkv, Nq, D], D = 64 or 128, bf16, any batch /
// head / row strides (views of a qkv projection pass without a copy). kv_len
// int32 [B] on the device ALREADY counts the new rows. Row i of batch row b
// goes to logical position
//   pos = decode_len(kv_len[b], Nq, capacity, causal = true) - Nq + i,
// in [0, capacity) because Nq <= len <= capacity: the position of query row i
// in the split-KV kernels, derived by the same function from the same integer.
//   * no table: the cache is [B, Hkv, Nmax, D], capacity = Nmax, and the row is
//     (b, kvh, pos);
//   * block_table int32 [B, max_pages]: the caches are page pools
//     [num_pages, Hkv, page_size, D], ANY page_size >= 1, capacity = max_pages *
//     page_size, and the row is (page, kvh, pos % page_size) with page =
//     block_table[b][pos / page_size] clamped to [0, num_pages - 1]; the index
//     pos / page_size <= (len - 1) / page_size is a live entry.
// Every address is therefore inside the caches whatever kv_len and the table
// hold. Nothing but the B * Nq * Hkv target rows of each cache is written.
// Two batch rows that a table sends to the same page row race; that table is
// the caller's mistake, as it is for the attention kernels that read it.
//
// Work split: the job is 2 * B * Nq * Hkv rows of D * 2 bytes and no math, so a
// lane moves one 16-byte piece of a K row and the same piece of the V row:
// kD / 8 = 8 or 16 lanes per row, a wave 8 or 4 rows, a block 32 or 16. Rows
// are numbered (b, i, kvh) with kvh fastest: in a qkv projection the Hkv rows
// of one token are adjacent, so a wave's reads are one contiguous run. Both
// loads are issued before either store. One launch, no LDS, no atomics, no
// host sync: positions come from kv_len and the table on the device, so the
// call is capturable and follows both across replays.
#pragma once

template <int kD>
kDecodeFn __global__ void __launch_bounds__(kAttnThreads) kvcache_append_kernel(
    const __hip_bfloat16* __restrict__ k_new, const __hip_bfloat16* __restrict__ v_new,
    __hip_bfloat16* __restrict__ k_cache, __hip_bfloat16* __restrict__ v_cache,
    const int* __restrict__ kv_len, const int* __restrict__ table, int Hkv, int Nq, int rows,
    int capacity, int max_pages, int page_size, int num_pages, Strides skn, Strides svn,
    Strides skc, Strides svc) {
  constexpr int kLanes = kD / 8; // 16-byte pieces of one row
  constexpr int kRows = kAttnThreads / kLanes; // rows of one block
  const int piece = threadIdx.x % kLanes;
  const int row = blockIdx.x * kRows + threadIdx.x / kLanes; // < rows + kRows <= INT32_MAX
  if (row >= rows) return;
  const int kvh = row % Hkv;
  const int i = (row / Hkv) % Nq;
  const int b = row / Hkv / Nq;
  const int pos = decode_len(kv_len, b, Nq, capacity, true) - Nq + i; // [0, capacity)
  int64_t page = b; // dense: one "page" of Nmax rows per batch row
  int r = pos;
  if (table != nullptr) {
    const int pg = pos / page_size; // < max_pages
    page = min(max(table[(int64_t)b * max_pages + pg], 0), num_pages - 1);
    r = pos - pg * page_size;
  }
  const int64_t src_k = (int64_t)b * skn.b + (int64_t)kvh * skn.h + (int64_t)i * skn.r + 8 * piece;
  const int64_t src_v = (int64_t)b * svn.b + (int64_t)kvh * svn.h + (int64_t)i * svn.r + 8 * piece;
  const bf16x8 kx = *(const bf16x8*)(k_new + src_k);
  const bf16x8 vx = *(const bf16x8*)(v_new + src_v);
  *(bf16x8*)(k_cache + page * skc.b + (int64_t)kvh * skc.h + (int64_t)r * skc.r + 8 * piece) = kx;
  *(bf16x8*)(v_cache + page * svc.b + (int64_t)kvh * svc.h + (int64_t)r * svc.r + 8 * piece) = vx;
}

void kvcache_append(at::Tensor k_new, at::Tensor v_new, at::Tensor k_cache, at::Tensor v_cache,
                    at::Tensor kv_len, c10::optional<at::Tensor> block_table) {
  TORCH_CHECK(k_new.is_cuda() && k_new.dim() == 4 && k_new.scalar_type() == at::kBFloat16 &&
                  (k_new.size(3) == kAttnD || k_new.size(3) == kAttnD128) && k_new.size(0) >= 1 &&
                  k_new.size(1) >= 1 && k_new.size(2) >= 1,
              "k_new must be a bf16 device tensor [B,Hkv,Nq,D] with B, Hkv, Nq >= 1 and D = 64 or 128");
  const int64_t B = k_new.size(0), Hkv = k_new.size(1), Nq = k_new.size(2), D = k_new.size(3);
  TORCH_CHECK(v_new.sizes() == k_new.sizes(), "v_new must be shaped like k_new");
  const bool paged = block_table.has_value();
  TORCH_CHECK(k_cache.dim() == 4 && (paged ? k_cache.size(0) >= 1 : k_cache.size(0) == B) &&
                  k_cache.size(1) == Hkv && k_cache.size(2) >= 1 && k_cache.size(3) == D,
              "k_cache must be [B,Hkv,Nmax,D] (with a block_table: [num_pages,Hkv,page_size,D]) "
              "with k_new's Hkv and D: got ", k_cache.sizes(), " for k_new ", k_new.sizes());
  TORCH_CHECK(v_cache.sizes() == k_cache.sizes(), "v_cache must be shaped like k_cache");
  int64_t capacity = k_cache.size(2), max_pages = 1;
  if (paged) {
    check_block_table(*block_table, k_new, B, "kvcache_append");
    max_pages = block_table->size(1);
    TORCH_CHECK(k_cache.size(0) <= INT32_MAX && max_pages <= INT32_MAX / k_cache.size(2),
                "kvcache_append: num_pages or max_pages * page_size too large");
    capacity = max_pages * k_cache.size(2);
  }
  TORCH_CHECK(capacity >= Nq, "the cache must hold the Nq new rows: capacity ", capacity, " < Nq ",
              Nq);
  TORCH_CHECK(capacity <= INT32_MAX && B * Nq * Hkv <= INT32_MAX - kAttnThreads,
              "kvcache_append: capacity or B*Nq*Hkv too large");
  for (const NamedTensor& a :
       {NamedTensor{"k_new", k_new}, {"v_new", v_new}, {"k_cache", k_cache}, {"v_cache", v_cache}}) {
    const at::Tensor& t = a.second;
    TORCH_CHECK(t.scalar_type() == at::kBFloat16 && t.device() == k_new.device() &&
                    t.stride(3) == 1,
                a.first, " must be bf16 on k_new's device with a contiguous last dim");
    // rows move as 16-byte vectors
    TORCH_CHECK((uintptr_t)t.data_ptr() % 16 == 0 && t.stride(0) % 8 == 0 && t.stride(1) % 8 == 0 &&
                    t.stride(2) % 8 == 0,
                a.first, " must be 16-byte aligned with batch/head/row strides that are multiples "
                         "of 8 elements");
  }
  TORCH_CHECK(kv_len.scalar_type() == at::kInt && kv_len.device() == k_new.device() &&
                  kv_len.dim() == 1 && kv_len.size(0) == B && kv_len.is_contiguous(),
              "kv_len must be int32 [B], contiguous, on k_new's device");

  const int64_t rows = B * Nq * Hkv;
  const int64_t rows_per_block = kAttnThreads / (D / 8);
  auto launch = [&](auto kernel) {
    hipLaunchKernelGGL(kernel, dim3((unsigned)ceil_div(rows, rows_per_block)), dim3(kAttnThreads),
                       0, c10::hip::getCurrentHIPStream(),
                       (const __hip_bfloat16*)k_new.data_ptr(),
                       (const __hip_bfloat16*)v_new.data_ptr(), (__hip_bfloat16*)k_cache.data_ptr(),
                       (__hip_bfloat16*)v_cache.data_ptr(), kv_len.data_ptr<int>(),
                       paged ? block_table->data_ptr<int>() : (const int*)nullptr, (int)Hkv,
                       (int)Nq, (int)rows, (int)capacity, (int)max_pages, (int)k_cache.size(2),
                       (int)k_cache.size(0), strides_of(k_new), strides_of(v_new),
                       strides_of(k_cache), strides_of(v_cache));
  };
  if (D == kAttnD128) launch(kvcache_append_kernel<kAttnD128>);
  else launch(kvcache_append_kernel<kAttnD>);
}
