// pybind11 / torch bindings of the gfx950 kernels (csrc/kernels/*.hip).
// Every op launches on the current HIP stream so it can be captured into a hipGraph
// (torch.cuda.CUDAGraph) and ordered with RCCL collectives issued by torch.distributed.
#ifdef LSA_BINDINGS_SELFTEST
// host-only build of the argument validation (csrc/tests/bindings_selftest.cpp, under ASan / UBSan on the CPU):
// CPU tensors stand in for device tensors, the launchers are stubs, no Python module
#include <ATen/ATen.h>
#include <hip/hip_runtime_api.h>
#else
#include <torch/extension.h>
#include <c10/hip/HIPStream.h>
#include <hip/hip_runtime.h>
#endif

#include "kernels/gemm_sk.h"
#include "kernels/lsa_epi.h"

extern "C" {
int lsa_gemm(const void* X, int ldx, int M, int K, const void* Wf, int N, void* out, int epi, int nb, int splitk,
             hipStream_t stream);
int lsa_add_rmsnorm(float* h, const float* parts, int nparts, long part_stride, const int* ids, const void* emb,
                    const int* row_idx, int write_h, const void* w, float eps, void* xn, int rows, int D,
                    int xf_mt, long long* ss_out, int ss_ld, int ss_nzero, void* x8, float* sx8, hipStream_t s);
int lsa_prefetch(const void* const* ptrs, const long* bytes, int nr, int wgs, hipStream_t s);
int lsa_res_add_ss(float* h, const float* parts, int nparts, long part_stride, void* xn, int rows, int D, int xf_mt,
                   long long* ss_out, hipStream_t s);
int lsa_a8_gemm(const void* X8, const void* s8, const float* sx, int M, int K, const void* Wq, const float* wscale,
                const void* Sw, int wk, int N, void* out, void* out_s8, int epi, int nb, int splitk, int waves, int depth,
                int xfo, const LsaEpi* ep, hipStream_t stream);
int lsa_quant_xf8(const void* x, int ldx, int M, int K, int MT, void* x8, float* sx, hipStream_t s);
int lsa_quant_xf8_blocks(const void* x, int ldx, int M, int K, int MT, int blk, void* x8, void* s8, hipStream_t s);
int lsa_gemm_ex(const void* X, int ldx, int M, int K, const void* Wf, int N, void* out, int epi, int nb, int splitk,
                int waves, int div, int xlds, const LsaEpi* ep, hipStream_t stream);
int lsa_fp8_gemm_ex(const void* X, int ldx, int M, int K, const void* Wq, const float* wscale, int N, void* out,
                    int epi, int nb, int splitk, int xfrag, const LsaEpi* ep, hipStream_t stream);
int lsa_rope_append(const void* qkv, const float* qkv_parts, int nparts, long part_stride, const int* pos, const int* tok_seq, const int* block_tables, int max_blocks,
                    const float* cos_t, const float* sin_t, void* q_out, void* kc, void* vc, float* ks, float* vs, int T,
                    int H, int Hkv, hipStream_t s);
int lsa_silu_mul(const void* g, const void* u, void* o, long n, hipStream_t s);
int lsa_attn_decode(const void* q, const void* kc, const void* vc, const int* block_tables, int max_blocks,
                    const int* pos, int B, int H, int Hkv, float scale, int chunk_blocks, int nsplit, int unsplit_max,
                    void* out, float* opart, float* mlpart, int* counters, int xf_mt, const float* qkv_parts, int nparts,
                    long part_stride,
                    const float* cos_t, const float* sin_t, const float* ks, const float* vs, void* out_s8,
                    const long long* rowss, float inv_k, float eps, hipStream_t s);
int lsa_gemm_rr(int K, const void* Wf, int N, void* out, int epi, int nb, int splitk, int waves, int div,
                const LsaRr* rr, hipStream_t stream);
int lsa_a8_gemm_rr(int K, const void* Wq, const float* wscale, const void* Sw, int wk, int N, void* out, void* out_s8,
                   int epi, int nb, int splitk, int waves, int depth, const LsaRr* rr, hipStream_t stream);
int lsa_kv8_dequant(const void* kc, const void* vc, const float* ks, const float* vs, const int* block_tables,
                    int max_blocks, const int* ctx_lens, int nseq, int Hkv, int mb, void* ko, void* vo, hipStream_t s);
int lsa_attn_prefill(const void* q, const void* kc, const void* vc, const int* block_tables, int max_blocks,
                     const int* cu_q, const int* ctx_lens, const int* work, int nwork, int H, int Hkv, float scale,
                     void* out, int xf_mt, hipStream_t s);
int lsa_argmax_commit(const float* logits, int B, int V, unsigned long long* part, int* out_tokens, int max_new,
                      int* gen_len, int* input_ids, int* positions, int* finished, const int* eos, int neos,
                      const int* limit, const int* eos_on, hipStream_t s);
int lsa_attn_verify(const void* q, const void* kc, const void* vc, const int* bt, int max_blocks, const int* pos0, int S,
                    int T, int H, int Hkv, float scale, int chunk_blocks, int nsplit, int unsplit_max, void* out, float* opart,
                    float* mlpart, int* counters, hipStream_t s, const float* ks = nullptr, const float* vs = nullptr);
int lsa_kv_copy_blocks(void* kv, void* scale, const int* pairs, int npairs, int planes, int nb, long long tile_bytes,
                       long long scale_bytes, hipStream_t s);
int lsa_kv_shift(void* kv, const int* moves, int n, int layers, int nb, int hkv, const float* cos_t, const float* sin_t,
                 int table_rows, hipStream_t s);
int lsa_kv_shift8(void* kv, float* kv_scale, const int* moves, int n, int layers, int nb, int hkv, const float* cos_t,
                  const float* sin_t, int table_rows, hipStream_t s);
int lsa_embed_rowscale(const float* h, const float* parts, int nparts, long part_stride, const int* tseq, const int* cu,
                       const int* meta, int n, int T, int D, float eps, float* rs, hipStream_t s);
int lsa_embed_pool(const float* h, const float* parts, int nparts, long part_stride, const int* cu, const int* meta,
                   int n, int T, int D, const float* rs, const void* gamma, float* acc, int nslots, hipStream_t s);
int lsa_embed_finish(const int* meta, int n, int D, const float* acc, float* out, int nslots, hipStream_t s);
int lsa_spec_draft(const int* prompt_tok, int prompt_ld, const int* prompt_len, const int* out_tokens, int max_new,
                   const int* gen_len, const int* input_ids, const int* positions, int rows, int k, int n_max, int n_min,
                   const int* forced, int nf, int forced_ld, int* spec_ids, int* spec_pos, int* spec_draft,
                   hipStream_t s);
int lsa_logprob_scan(const float* logits, int B, int V, const int* lp_k, const int* finished, const int* gen_len,
                     float* lp_raw, float* lp_ms, unsigned long long* lp_cand, int* lp_n0, hipStream_t s);
int lsa_logprob_commit(const float* lp_raw, int B, int V, const float* lp_ms, const unsigned long long* lp_cand,
                       const int* lp_k, int* lp_n0, const int* gen_len, const int* out_tokens, int max_new, float* lp_tok,
                       int* lp_ids, float* lp_top, int kcap, hipStream_t s);
int lsa_spec_logprob_scan(const float* logits, int S, int T, int V, const int* lp_k, const int* finished,
                          const int* gen_len, float* sp_raw, float* sp_ms, unsigned long long* sp_cand, int* lp_n0,
                          hipStream_t st);
int lsa_spec_logprob_commit(const float* sp_raw, int S, int T, int V, const float* sp_ms,
                            const unsigned long long* sp_cand, const int* lp_k, const int* lp_n0, const int* gen_len,
                            const int* out_tokens, int max_new, float* lp_tok, int* lp_ids, float* lp_top, int kcap,
                            hipStream_t st);
int lsa_prompt_logprob_scan(const float* logits, int R, int V, const int* targets, int any_k, float* ms,
                            unsigned long long* cand, hipStream_t s);
int lsa_prompt_logprob_commit(const float* logits, int R, int V, const float* ms, const unsigned long long* cand,
                              const int* targets, const int* row_k, int any_k, float* dst_tok, int* dst_ids,
                              float* dst_top, int kcap, hipStream_t s);
int lsa_dfa_mask(float* logits, int B, int V, const int* tok_off, const uint8_t* tok_blob, const uint8_t* cls,
                 const uint16_t* trans, const uint8_t* accept, const int* g_dim, const int* g_on, int* g_state,
                 const int* g_base, const int* rows, const int* gen_len, const int* input_ids, const int* finished,
                 const int* eos, int neos, hipStream_t s);
int lsa_dfa_mask_verify(float* logits, int T, int V, const int* tok_off, const uint8_t* tok_blob, const uint8_t* cls,
                        const uint16_t* trans, const uint8_t* accept, const int* g_dim, const int* g_on, int* g_state,
                        const int* g_base, int r, const int* gen_len, const int* input_ids, const int* finished,
                        const int* eos, int neos, const int* draft, int* g_spec, hipStream_t s);
int lsa_dfa_mask_verify_batch(float* logits, int S, int T, int V, const int* tok_off, const uint8_t* tok_blob,
                              const uint8_t* cls, const uint16_t* trans, const uint8_t* accept, const int* g_dim,
                              const int* g_on, int* g_state, const int* g_base, int r, const int* gen_len,
                              const int* input_ids, const int* finished, const int* eos, int neos, const int* draft,
                              int* g_spec, hipStream_t s);
int lsa_dfa_spec_advance_batch(const int* g_on, int* g_state, const int* g_spec, const int* gen_len, int r, int S, int k,
                               hipStream_t s);
int lsa_dfa_spec_advance(const int* g_on, int* g_state, const int* g_spec, const int* gen_len, int r, int k,
                         hipStream_t s);
int lsa_spec_commit(const float* logits, int S, int T, int V, unsigned long long* part, const int* draft,
                    long long* stats, int* out_tokens, int max_new, int* gen_len, int* input_ids, int* positions, int* finished,
                    const int* eos, int neos, const int* limit, const int* eos_on, hipStream_t s);
int lsa_sample_commit(float* logits, int B, int V, unsigned long long* part, unsigned long long* cand, int* hist,
                      int window, const float* penalty, const int* last_n, const float* temperature, const int* top_k,
                      const float* top_p, const unsigned long long* seeds, int* out_tokens, int max_new, int* gen_len,
                      int* input_ids, int* positions, int* finished, const int* eos, int neos, const int* limit,
                      const int* eos_on, const float* presence, const float* frequency, const float* min_p,
                      hipStream_t s);
int lsa_spec_sample_commit(float* logits, int S, int T, int V, const int* draft, long long* stats, int* hist, int window,
                           const float* penalty, const int* last_n, const float* temperature, const int* top_k,
                           const float* top_p, const unsigned long long* seeds, int* out_tokens, int max_new,
                           int* gen_len, int* input_ids, int* positions, int* finished, const int* eos, int neos,
                           const int* limit, const int* eos_on, unsigned long long* part, unsigned long long* cand,
                           int* picks, const float* presence, const float* frequency, const float* min_p, hipStream_t s);
int lsa_fp8_gemm(const void* X, int ldx, int M, int K, const void* Wq, const float* wscale, int N, void* out, int epi,
                 int nb, int splitk, hipStream_t stream);
int lsa_fp8_dequant(const void* Wq, const float* wscale, int N, int K, void* Wf, hipStream_t s);
int lsa_gemm_cfg(const void* X, int ldx, int M, int K, const void* Wf, int N, void* out, int epi, int nb, int splitk,
                 int waves, int div, int xlds, hipStream_t stream);
int lsa_fp8_gemm_cfg(const void* X, int ldx, int M, int K, const void* Wq, const float* wscale, int N, void* out,
                     int epi, int nb, int splitk, int xfrag, hipStream_t stream);
void lsa_gemm_sk_epilogue(int mode);
void lsa_gemm_sk_nbuf(int n);
void lsa_gemm_sk_one_phase(int on);
void lsa_rmsnorm_xf_tile_min(int rows);
int lsa_gemm_sk_rope(const void* X, int ldx, int M, int K, const void* Wf, int N, float* ws, int* tickets, int ncu,
                     int min_share, int cfg, const int* pos, const int* tok_seq, const int* block_tables,
                     int max_blocks, const float* cos_t, const float* sin_t, void* q_out, void* kc, void* vc, int H,
                     int Hkv, int xf, int* grid_out, int* cfg_out, hipStream_t stream);
int lsa_gemm_sk(const void* X, int ldx, int M, int K, const void* Wf, int N, void* out, int epi, float* ws,
                int* tickets, int ncu, int min_share, int cfg, int xf, int* grid_out, int* cfg_out, hipStream_t stream);
int lsa_silu_parts(const float* parts, int nparts, long part_stride, int M, int F, void* out, hipStream_t s);
int lsa_silu_bf16(const void* y, int M, int F, void* out, hipStream_t s);
void lsa_fp8_gemm_knobs(int waves, int depth);
int lsa_attn_prefill32(const void* q, const void* kc, const void* vc, const int* block_tables, int max_blocks,
                       const int* cu_q, const int* ctx_lens, const int* work, int nwork, int H, int Hkv, float scale,
                       void* out, int ng, int xf_mt, hipStream_t s);
int lsa_quant_rows_fp8(const void* x, int ldx, int M, int K, void* x8, int ld8, float* sx, hipStream_t s);
int lsa_fp8_gemm_t256(const void* X8, int ldx, const float* sx, int M, int K, const void* Wq, const float* sw, int N,
                      void* out, int epi, int splitk, hipStream_t stream);
int lsa_ar_alloc(size_t bytes, void** out);
int lsa_ar_free(void* p);
int lsa_ar_handle(void* p, char* out64);
int lsa_ar_open(const char* in64, void** out);
int lsa_ar_close(void* p);
int lsa_ar_max_world();
int lsa_prefill_qblock();
int lsa_ar_wallclock_khz(int* out);
int lsa_ar_header_bytes();
int lsa_ar_run(float* data, long n, float* out, uint8_t* const* regions, int rank, int world, size_t maxb,
               int nblocks, long long timeout_ticks, int* err, int nslab, long slab_stride, const float* res_h,
               void* res_xn, long long* res_ss, int res_d, int res_xmt, int mode, hipStream_t s);
int lsa_fp4_gemm_ex(const void* X, int ldx, int M, int K, const void* Wq, const void* S, int N, void* out, int epi,
                    int nb, int splitk, int waves, int xfrag, const LsaEpi* ep, hipStream_t stream);
int lsa_fp4_dequant(const void* Wq, const void* S, int N, int K, void* Wf, hipStream_t s);
int lsa_q4_gemm_ex(const void* X, int ldx, int M, int K, const void* Wq, const void* D, int N, void* out, int epi,
                   int nb, int splitk, int waves, int xfrag, const LsaEpi* ep, hipStream_t stream);
int lsa_q4_dequant(const void* Wq, const void* D, int N, int K, void* Wf, hipStream_t s);
int lsa_gemm_z12(const void* X, int M, int K, const void* lo, const void* hi, const void* esc, int base, int N,
                 void* out, int epi, int nb, int splitk, int waves, int div, const LsaEpi* ep, hipStream_t stream);
}

namespace {

#ifdef LSA_BINDINGS_SELFTEST
hipStream_t cur_stream() { return nullptr; }
bool on_dev(const at::Tensor& t) { return t.defined(); }
#else
hipStream_t cur_stream() { return c10::hip::getCurrentHIPStream().stream(); }
bool on_dev(const at::Tensor& t) { return t.is_cuda(); }
#endif

void check(int rc, const char* what) { TORCH_CHECK(rc == 0, "lsa kernel '", what, "' failed: rc=", rc); }

void need(const at::Tensor& t, at::ScalarType dt, const char* name) {
  TORCH_CHECK(on_dev(t), name, " must be a GPU tensor");
  TORCH_CHECK(t.scalar_type() == dt, name, " has dtype ", t.scalar_type(), ", expected ", dt);
}

// paged KV cache operands: bf16 [nblk, Hkv, 64, 128], or fp8 (uint8 e4m3 bytes, same shape) with f32
// per-(token, kv-head) scales [nblk, Hkv, 64]
void check_cache(const at::Tensor& kc, const at::Tensor& vc, const c10::optional<at::Tensor>& ks,
                 const c10::optional<at::Tensor>& vs) {
  TORCH_CHECK(ks.has_value() == vs.has_value(), "fp8 cache needs both K and V scales");
  TORCH_CHECK(kc.dim() == 4 && kc.size(2) == 64 && kc.size(3) == 128 && kc.sizes() == vc.sizes() &&
                  kc.is_contiguous() && vc.is_contiguous(), "cache must be contiguous [nblk, Hkv, 64, 128]");
  const at::ScalarType dt = ks.has_value() ? at::kByte : at::kBFloat16;
  need(kc, dt, "kc");
  need(vc, dt, "vc");
  if (ks.has_value()) {
    need(*ks, at::kFloat, "ks");
    need(*vs, at::kFloat, "vs");
    TORCH_CHECK(ks->numel() == kc.numel() / 128 && vs->numel() == kc.numel() / 128 && ks->is_contiguous() &&
                    vs->is_contiguous(), "fp8 cache scales must be contiguous [nblk, Hkv, 64]");
  }
}

template <typename T>
T* ptr(const c10::optional<at::Tensor>& t) {
  return t.has_value() ? reinterpret_cast<T*>(t->data_ptr()) : nullptr;
}

// Decode epilogue extensions (kernels/lsa_epi.h): rowss = per-row sum of squares of the un-normalised
// input rows (RMS row scale with eps, 1/K); epi 3 (residual) adds into h [M, N] f32, writes bf16(h) to
// xout (fragment-major with xmt row tiles, or row-major when xmt == 0) and accumulates sum h^2 into ss_out.
struct EpiOpts {
  LsaEpi e{};
  bool on = false;
};

EpiOpts epi_opts(int64_t epi, int64_t M, int64_t N, int64_t K, const c10::optional<at::Tensor>& rowss, double eps,
                 const c10::optional<at::Tensor>& h, const c10::optional<at::Tensor>& xout, int64_t xmt,
                 const c10::optional<at::Tensor>& ss_out, const c10::optional<at::Tensor>& tickets, int64_t ncols) {
  EpiOpts o;
  if (rowss.has_value()) {
    need(*rowss, at::kLong, "rowss");
    TORCH_CHECK(rowss->numel() >= M, "rowss too small");
    o.e.rowss = reinterpret_cast<const long long*>(rowss->data_ptr<int64_t>());
    o.e.inv_k = 1.0f / (float)K;
    o.e.eps = (float)eps;
    o.on = true;
  }
  if (epi == 3) {
    TORCH_CHECK(h.has_value() && xout.has_value() && ss_out.has_value(), "residual epilogue needs h, xout, ss_out");
    need(*h, at::kFloat, "h");
    need(*xout, at::kBFloat16, "xout");
    need(*ss_out, at::kLong, "ss_out");
    TORCH_CHECK(h->is_contiguous() && h->numel() >= M * N, "h must be a contiguous [M, N] f32 tensor");
    TORCH_CHECK(ss_out->numel() >= M, "ss_out too small");
    TORCH_CHECK(xout->numel() >= (xmt ? xmt * 16 * N : M * N), "xout too small");
    o.e.h = h->data_ptr<float>();
    o.e.ldh = (int)N;
    o.e.xout = reinterpret_cast<uint16_t*>(xout->data_ptr());
    o.e.xmt = (int)xmt;
    o.e.ss_out = reinterpret_cast<long long*>(ss_out->data_ptr<int64_t>());
    if (tickets.has_value()) {
      need(*tickets, at::kInt, "tickets");
      TORCH_CHECK(tickets->numel() >= ncols, "tickets: one counter per 16-column block needed");
      o.e.tickets = tickets->data_ptr<int>();
    }
    o.on = true;
  }
  return o;
}

void check_out(int64_t epi, const at::Tensor& out, int64_t splitk, int64_t M, int64_t N, int64_t mt_silu) {
  if (epi == 3 && splitk <= 1) return;  // the residual epilogue writes through h / xout
  if (epi == 1 || epi == 3) {  // f32 slabs (split-K residual: the partials of the splits)
    need(out, at::kFloat, "out");
    TORCH_CHECK(out.numel() >= splitk * M * N, "f32 out too small");
  } else {
    need(out, at::kBFloat16, "out");
    TORCH_CHECK(out.numel() >= (epi == 2 ? (mt_silu ? mt_silu * 16 : M) * (N / 2) : M * N), "bf16 out too small");
  }
}

// out = x @ W^T with W in fragment-major layout (see kernels/gemm.hip)
void gemm(const at::Tensor& x, const at::Tensor& wf, int64_t N, at::Tensor& out, int64_t epi, int64_t nb,
          int64_t splitk, int64_t waves, int64_t div, int64_t xlds, const c10::optional<at::Tensor>& rowss,
          double eps, const c10::optional<at::Tensor>& h, const c10::optional<at::Tensor>& xout, int64_t xmt,
          const c10::optional<at::Tensor>& ss_out, const c10::optional<at::Tensor>& tickets) {
  need(x, at::kBFloat16, "x");
  need(wf, at::kBFloat16, "wf");
  TORCH_CHECK(x.dim() == 2 && x.stride(1) == 1, "x must be a row-major matrix");
  const int M = x.size(0), K = x.size(1);
  TORCH_CHECK(wf.numel() == N * K, "weight numel mismatch: ", wf.numel(), " vs ", N, "x", K);
  const EpiOpts eo = epi_opts(epi, M, N, K, rowss, eps, h, xout, xmt, ss_out, tickets, N / 16);
  if (eo.on) {
    check_out(epi, out, splitk, M, N, 0);
    check(lsa_gemm_ex(x.data_ptr(), x.stride(0), M, K, wf.data_ptr(), N, out.data_ptr(), epi, nb, splitk, waves, div,
                      xlds, &eo.e, cur_stream()),
          "gemm");
    return;
  }
  if (epi == 1) {
    need(out, at::kFloat, "out");
    TORCH_CHECK(out.numel() >= splitk * M * N, "f32 out too small");
  } else {
    need(out, at::kBFloat16, "out");
    TORCH_CHECK(out.numel() >= M * (epi == 2 ? N / 2 : N), "bf16 out too small");
  }
  check(lsa_gemm_cfg(x.data_ptr(), x.stride(0), M, K, wf.data_ptr(), N, out.data_ptr(), epi, nb, splitk, waves, div,
                     xlds, cur_stream()),
        "gemm");
}

// Batch-1 decode GEMM with the residual-reduce prologue (kernels/gemm.hip, lsa_epi.h LsaRr): X = h + sum_s parts[s]
// (h f32 [K]; parts f32 [np, 1, K] split-K slabs), h_out = X.  epi 1: f32 slabs [splitk, 1, N], the column-0
// workgroups add each K slice's sum of X^2 (Q24) into ss_out[0] (the slab consumer applies the row scale);
// epi 2: SiLU(gate) * up bf16 [1, N / 2] with the RMS row scale from the workgroup's own full-row sum (splitk 1).
void gemm_rr(const at::Tensor& h, const at::Tensor& parts, at::Tensor& h_out, const at::Tensor& wf, int64_t N,
             at::Tensor& out, int64_t epi, int64_t nb, int64_t splitk, int64_t waves, int64_t div,
             const c10::optional<at::Tensor>& ss_out, double eps) {
  need(h, at::kFloat, "h");
  need(h_out, at::kFloat, "h_out");
  need(parts, at::kFloat, "parts");
  need(wf, at::kBFloat16, "wf");
  const int64_t K = h.numel();
  TORCH_CHECK(h.is_contiguous() && h_out.is_contiguous() && h_out.numel() >= K, "gemm_rr: h / h_out contiguous [K]");
  TORCH_CHECK(h.data_ptr() != h_out.data_ptr(), "gemm_rr: h_out must not alias h (other workgroups still read h)");
  TORCH_CHECK(parts.dim() == 3 && parts.size(1) == 1 && parts.size(2) == K && parts.stride(2) == 1 &&
                  parts.stride(1) == K, "gemm_rr: parts must be [np, 1, K] slabs");
  TORCH_CHECK(wf.numel() == N * K, "gemm_rr: weight numel mismatch");
  TORCH_CHECK(epi == 1 || epi == 2, "gemm_rr: f32 slabs or silu");
  check_out(epi, out, splitk, 1, N, 0);
  LsaRr rr{};
  rr.h = h.data_ptr<float>();
  rr.parts = parts.data_ptr<float>();
  rr.pstride = parts.stride(0);
  rr.np = (int)parts.size(0);
  rr.h_out = h_out.data_ptr<float>();
  rr.local = epi == 2 ? 1 : 0;
  rr.inv_k = 1.0f / (float)K;
  rr.eps = (float)eps;
  if (epi == 1) {
    TORCH_CHECK(ss_out.has_value(), "gemm_rr: f32 slabs need ss_out");
    need(*ss_out, at::kLong, "ss_out");
    rr.ss_out = reinterpret_cast<long long*>(ss_out->data_ptr<int64_t>());
  }
  check(lsa_gemm_rr((int)K, wf.data_ptr(), (int)N, out.data_ptr(), (int)epi, (int)nb, (int)splitk, (int)waves, (int)div,
                    &rr, cur_stream()),
        "gemm_rr");
}

// same, with X in the fragment-major activation layout (ops.to_xfrag): xf holds ceil(M/16) row tiles
void gemm_xf(const at::Tensor& xf, int64_t M, int64_t K, const at::Tensor& wf, int64_t N, at::Tensor& out,
             int64_t epi, int64_t nb, int64_t splitk, int64_t waves, int64_t div,
             const c10::optional<at::Tensor>& rowss, double eps, const c10::optional<at::Tensor>& h,
             const c10::optional<at::Tensor>& xout, int64_t xmt, const c10::optional<at::Tensor>& ss_out, const c10::optional<at::Tensor>& tickets) {
  need(xf, at::kBFloat16, "xf");
  need(wf, at::kBFloat16, "wf");
  TORCH_CHECK(M >= 1 && M <= 64 && K % 32 == 0, "gemm_xf: M in 1..64, K % 32 == 0");
  const int64_t mt = M <= 16 ? 1 : (M <= 32 ? 2 : 4);
  TORCH_CHECK(xf.is_contiguous() && xf.numel() >= mt * 16 * K, "xf too small for M=", M, " K=", K);
  TORCH_CHECK(wf.numel() == N * K, "weight numel mismatch");
  check_out(epi, out, splitk, M, N, mt);
  const EpiOpts eo = epi_opts(epi, M, N, K, rowss, eps, h, xout, xmt, ss_out, tickets, N / 16);
  check(lsa_gemm_ex(xf.data_ptr(), K, M, K, wf.data_ptr(), N, out.data_ptr(), epi, nb, splitk, waves, div, 2,
                    eo.on ? &eo.e : nullptr, cur_stream()),
        "gemm_xf");
}

// gemm_xf at 17..32 rows over the lossless 12-bit weight stream (kernels/gemm_z12.hip; lo / hi / esc / base:
// ops.pack_z12 of the [N, K] bf16 weight): bit-identical to gemm_xf at the same (nb, splitk, waves, div).
// Epilogues bf16, f32 slabs, SiLU; row scale; no residual epilogue.
void z12_gemm_xf(const at::Tensor& xf, int64_t M, int64_t K, const at::Tensor& lo, const at::Tensor& hi,
                 const at::Tensor& esc, int64_t base, int64_t N, at::Tensor& out, int64_t epi, int64_t nb,
                 int64_t splitk, int64_t waves, int64_t div, const c10::optional<at::Tensor>& rowss, double eps) {
  need(xf, at::kBFloat16, "xf");
  need(lo, at::kByte, "lo");
  need(hi, at::kByte, "hi");
  need(esc, at::kInt, "esc");
  TORCH_CHECK(M > 16 && M <= 32 && K >= 32 && K % 32 == 0 && N >= 16 && N % 16 == 0,
              "z12_gemm_xf: M in 17..32, K % 32 == 0, N % 16 == 0");
  TORCH_CHECK(epi >= 0 && epi <= 2, "z12_gemm_xf: epilogue bf16 (0), f32 (1) or silu (2)");
  TORCH_CHECK(base >= 1 && base <= 120, "z12_gemm_xf: base out of range");
  TORCH_CHECK(splitk >= 1 && splitk <= K / 32 && (epi == 1 || splitk == 1), "z12_gemm_xf: bad splitk");
  TORCH_CHECK(xf.is_contiguous() && xf.numel() >= 2 * 16 * K, "xf too small for M=", M, " K=", K);
  TORCH_CHECK(lo.is_contiguous() && hi.is_contiguous() && esc.is_contiguous() && lo.numel() == N * K &&
                  hi.numel() == N * K / 2 && esc.numel() == (N / 16) * (K / 32) * 4,
              "z12 planes do not match N x K");
  check_out(epi, out, splitk, M, N, 2);
  // the fragment-major SiLU output is written in whole 32-column k-steps of two row tiles
  TORCH_CHECK(epi != 2 || out.numel() >= 32 * ((N / 2 + 31) / 32 * 32), "z12_gemm_xf: silu out too small");
  const EpiOpts eo = epi_opts(epi, M, N, K, rowss, eps, c10::nullopt, c10::nullopt, 0, c10::nullopt, c10::nullopt, 0);
  check(lsa_gemm_z12(xf.data_ptr(), (int)M, (int)K, lo.data_ptr(), hi.data_ptr(), esc.data_ptr(), (int)base, (int)N,
                     out.data_ptr(), (int)epi, (int)nb, (int)splitk, (int)waves, (int)div, eo.on ? &eo.e : nullptr,
                     cur_stream()),
        "z12_gemm_xf");
}

// fp8 weights, activations in the fragment-major decode layout (ops.to_xfrag), M <= 64
void fp8_gemm_xf(const at::Tensor& xf, int64_t M, int64_t K, const at::Tensor& wq, const at::Tensor& wscale, int64_t N,
                 at::Tensor& out, int64_t epi, int64_t nb, int64_t splitk, int64_t waves, int64_t depth,
                 const c10::optional<at::Tensor>& rowss,
                 double eps, const c10::optional<at::Tensor>& h, const c10::optional<at::Tensor>& xout, int64_t xmt,
                 const c10::optional<at::Tensor>& ss_out, const c10::optional<at::Tensor>& tickets) {
  need(xf, at::kBFloat16, "xf");
  need(wscale, at::kFloat, "wscale");
  TORCH_CHECK(on_dev(wq) && wq.element_size() == 1 && wq.numel() == N * K, "wq must be N*K fp8 bytes");
  TORCH_CHECK(M >= 1 && M <= 64 && K % 64 == 0, "fp8_gemm_xf: M in 1..64, K % 64 == 0");
  const int64_t mt = M <= 16 ? 1 : (M <= 32 ? 2 : 4);
  TORCH_CHECK(xf.is_contiguous() && xf.numel() >= mt * 16 * K, "xf too small");
  check_out(epi, out, splitk, M, N, mt);
  const EpiOpts eo = epi_opts(epi, M, N, K, rowss, eps, h, xout, xmt, ss_out, tickets, N / 16);
  lsa_fp8_gemm_knobs((int)waves, (int)depth);
  check(lsa_fp8_gemm_ex(xf.data_ptr(), K, M, K, wq.data_ptr(), wscale.data_ptr<float>(), N, out.data_ptr(), epi, nb,
                        splitk, 1, eo.on ? &eo.e : nullptr, cur_stream()),
        "fp8_gemm_xf");
}

// W8A8 / W4A8 decode GEMM (kernels/gemm_fp8a.hip): x8 e4m3 activations in the xf8 layout with per-row f32 scales
// sx and / or per-lane-block E8M0 scales s8; fp8 weights (wscale per channel) or MXFP4 weights (wsc8 = their E8M0
// block-scale words).  xfo 2: the SiLU output as e4m3 + E8M0 blocks into (out, out_s8).
void a8_gemm(const at::Tensor& x8, const c10::optional<at::Tensor>& s8, const c10::optional<at::Tensor>& sx, int64_t M,
             int64_t K, const at::Tensor& wq, const c10::optional<at::Tensor>& wscale,
             const c10::optional<at::Tensor>& wsc8, int64_t N, at::Tensor& out, const c10::optional<at::Tensor>& out_s8,
             int64_t epi, int64_t nb, int64_t splitk, int64_t waves, int64_t depth, int64_t xfo,
             const c10::optional<at::Tensor>& rowss, double eps) {
  const bool fp4 = wsc8.has_value();
  TORCH_CHECK(fp4 != wscale.has_value(), "a8_gemm: exactly one of wscale (fp8) / wsc8 (mxfp4)");
  TORCH_CHECK(M >= 1 && M <= 64 && K % 128 == 0 && N % 16 == 0, "a8_gemm: M in 1..64, K % 128 == 0, N % 16 == 0");
  TORCH_CHECK(epi == 1 || epi == 2, "a8_gemm: f32 slabs or silu");
  TORCH_CHECK(on_dev(wq) && wq.element_size() == 1 && wq.numel() == (fp4 ? N * K / 2 : N * K), "a8_gemm: weight bytes");
  if (fp4) {
    TORCH_CHECK(on_dev(*wsc8) && wsc8->numel() * wsc8->element_size() >= (N / 16) * ((K / 128 + 3) / 4) * 256,
                "a8_gemm: mxfp4 scales too small");
  } else {
    need(*wscale, at::kFloat, "wscale");
    TORCH_CHECK(wscale->numel() >= N, "a8_gemm: wscale too small");
  }
  const int64_t mt = M <= 16 ? 1 : (M <= 32 ? 2 : 4);
  TORCH_CHECK(on_dev(x8) && x8.element_size() == 1 && x8.is_contiguous() && x8.numel() >= mt * 16 * K, "x8 too small");
  TORCH_CHECK(s8.has_value() || sx.has_value(), "a8_gemm: per-row (sx) and / or block (s8) activation scales");
  if (s8.has_value())
    TORCH_CHECK(on_dev(*s8) && s8->element_size() == 1 && s8->numel() >= mt * 64 * (K / 128), "s8 too small");
  if (sx.has_value()) {
    need(*sx, at::kFloat, "sx");
    TORCH_CHECK(sx->numel() >= M, "sx too small");
  }
  if (epi == 2 && xfo == 2) {
    TORCH_CHECK(on_dev(out) && out.element_size() == 1 && out.numel() >= mt * 16 * (N / 2), "e4m3 SiLU out too small");
    TORCH_CHECK(out_s8.has_value() && on_dev(*out_s8) && out_s8->element_size() == 1 &&
                    out_s8->numel() >= mt * 64 * (N / 2 / 128) && (N / 2) % 128 == 0,
                "a8_gemm: e4m3 SiLU output needs out_s8 (and N / 2 % 128 == 0)");
  } else {
    check_out(epi, out, splitk, M, N, xfo ? mt : 0);
  }
  const EpiOpts eo = epi_opts(epi, M, N, K, rowss, eps, c10::nullopt, c10::nullopt, 0, c10::nullopt, c10::nullopt, N / 16);
  check(lsa_a8_gemm(x8.data_ptr(), s8.has_value() ? s8->data_ptr() : nullptr,
                    sx.has_value() ? sx->data_ptr<float>() : nullptr, M, K, wq.data_ptr(),
                    fp4 ? nullptr : wscale->data_ptr<float>(), fp4 ? wsc8->data_ptr() : nullptr, fp4 ? 1 : 0, N,
                    out.data_ptr(), out_s8.has_value() ? out_s8->data_ptr() : nullptr, epi, nb, splitk, waves, depth, xfo,
                    eo.on ? &eo.e : nullptr, cur_stream()),
        "a8_gemm");
}

// W8A8 / W4A8 batch-1 decode GEMM with the residual-reduce prologue (kernels/gemm_fp8a.hip RR): X = h + sum_s parts[s]
// quantised in the prologue (e4m3, one E8M0 scale per 32 k); h_out = X.  epi 1: f32 slabs [splitk, 1, N] (ss_out[0] +=
// sum X^2, the slab consumer scales the row); epi 2: the e4m3 SiLU output in the xf8 layout + E8M0 blocks in out_s8
// (splitk 1, the row scale from the workgroup's own full-row sum).
void a8_gemm_rr(const at::Tensor& h, const at::Tensor& parts, at::Tensor& h_out, const at::Tensor& wq,
                const c10::optional<at::Tensor>& wscale, const c10::optional<at::Tensor>& wsc8, int64_t N, at::Tensor& out,
                const c10::optional<at::Tensor>& out_s8, int64_t epi, int64_t nb, int64_t splitk, int64_t waves,
                int64_t depth, const c10::optional<at::Tensor>& ss_out, double eps) {
  const bool fp4 = wsc8.has_value();
  TORCH_CHECK(fp4 != wscale.has_value(), "a8_gemm_rr: exactly one of wscale (fp8) / wsc8 (mxfp4)");
  need(h, at::kFloat, "h");
  need(h_out, at::kFloat, "h_out");
  need(parts, at::kFloat, "parts");
  const int64_t K = h.numel();
  TORCH_CHECK(K % 128 == 0 && N % 16 == 0, "a8_gemm_rr: K % 128 == 0, N % 16 == 0");
  TORCH_CHECK(h.is_contiguous() && h_out.is_contiguous() && h_out.numel() >= K, "a8_gemm_rr: h / h_out contiguous [K]");
  TORCH_CHECK(h.data_ptr() != h_out.data_ptr(), "a8_gemm_rr: h_out must not alias h");
  TORCH_CHECK(parts.dim() == 3 && parts.size(1) == 1 && parts.size(2) == K && parts.stride(2) == 1 &&
                  parts.stride(1) == K, "a8_gemm_rr: parts must be [np, 1, K] slabs");
  TORCH_CHECK(on_dev(wq) && wq.element_size() == 1 && wq.numel() == (fp4 ? N * K / 2 : N * K), "a8_gemm_rr: weight bytes");
  if (fp4) {
    TORCH_CHECK(on_dev(*wsc8) && wsc8->numel() * wsc8->element_size() >= (N / 16) * ((K / 128 + 3) / 4) * 256,
                "a8_gemm_rr: mxfp4 scales too small");
  } else {
    need(*wscale, at::kFloat, "wscale");
    TORCH_CHECK(wscale->numel() >= N, "a8_gemm_rr: wscale too small");
  }
  TORCH_CHECK(epi == 1 || epi == 2, "a8_gemm_rr: f32 slabs or the e4m3 SiLU output");
  if (epi == 2) {
    TORCH_CHECK(on_dev(out) && out.element_size() == 1 && out.numel() >= 16 * (N / 2), "a8_gemm_rr: e4m3 SiLU out too small");
    TORCH_CHECK(out_s8.has_value() && on_dev(*out_s8) && out_s8->element_size() == 1 && out_s8->numel() >= 64 * (N / 2 / 128) &&
                    (N / 2) % 128 == 0, "a8_gemm_rr: the e4m3 SiLU output needs out_s8 (and N / 2 % 128 == 0)");
  } else {
    check_out(epi, out, splitk, 1, N, 0);
  }
  LsaRr rr{};
  rr.h = h.data_ptr<float>();
  rr.parts = parts.data_ptr<float>();
  rr.pstride = parts.stride(0);
  rr.np = (int)parts.size(0);
  rr.h_out = h_out.data_ptr<float>();
  rr.local = epi == 2 ? 1 : 0;
  rr.inv_k = 1.0f / (float)K;
  rr.eps = (float)eps;
  if (epi == 1) {
    TORCH_CHECK(ss_out.has_value(), "a8_gemm_rr: f32 slabs need ss_out");
    need(*ss_out, at::kLong, "ss_out");
    rr.ss_out = reinterpret_cast<long long*>(ss_out->data_ptr<int64_t>());
  }
  check(lsa_a8_gemm_rr((int)K, wq.data_ptr(), fp4 ? nullptr : wscale->data_ptr<float>(),
                       fp4 ? wsc8->data_ptr() : nullptr, fp4 ? 1 : 0, (int)N, out.data_ptr(),
                       out_s8.has_value() ? out_s8->data_ptr() : nullptr, (int)epi, (int)nb, (int)splitk, (int)waves,
                       (int)depth, &rr, cur_stream()),
        "a8_gemm_rr");
}

void quant_xf8_blocks(const at::Tensor& x, int64_t mt, int64_t blk, at::Tensor& x8, at::Tensor& s8) {
  need(x, at::kBFloat16, "x");
  TORCH_CHECK(x.dim() == 2 && x.stride(1) == 1, "x must be a row-major matrix");
  const int M = x.size(0), K = x.size(1);
  TORCH_CHECK(on_dev(x8) && x8.element_size() == 1 && x8.numel() >= mt * 16 * K, "x8 too small");
  TORCH_CHECK(on_dev(s8) && s8.element_size() == 1 && s8.numel() >= mt * 64 * (K / 128), "s8 too small");
  check(lsa_quant_xf8_blocks(x.data_ptr(), x.stride(0), M, K, (int)mt, (int)blk, x8.data_ptr(), s8.data_ptr(),
                             cur_stream()),
        "quant_xf8_blocks");
}

void quant_xf8(const at::Tensor& x, int64_t mt, at::Tensor& x8, at::Tensor& sx) {
  need(x, at::kBFloat16, "x");
  need(sx, at::kFloat, "sx");
  TORCH_CHECK(x.dim() == 2 && x.stride(1) == 1, "x must be a row-major matrix");
  const int M = x.size(0), K = x.size(1);
  TORCH_CHECK(on_dev(x8) && x8.element_size() == 1 && x8.numel() >= mt * 16 * K && sx.numel() >= M, "x8 / sx too small");
  check(lsa_quant_xf8(x.data_ptr(), x.stride(0), M, K, (int)mt, x8.data_ptr(), sx.data_ptr<float>(), cur_stream()),
        "quant_xf8");
}

// large-M (prefill) linear layer on the stream-K 256x256 tile kernel (kernels/gemm_tile256.hip).  epi: 0 bf16 [M][N],
// 1 f32 [M][N], 2 SiLU(gate) * up bf16 [M][N / 2], 3 h f32 [M][N] += x @ W^T.  ws / tickets: the per-stream
// workspace (ops._sk_workspace).  cfg: -1 = the kernel's cost model, else a tile configuration index (+ 8: whole
// tiles only; + 16 + 32 * mode: that epilogue mode for this call).  xf: + 1 x is a flat buffer in the fragment-major
// layout (ops.to_xfrag) of ``rows`` rows, + 2 the SiLU output is written in it.  Returns grid * 16 + the configuration
// used.
// rows / K of a stream-K GEMM's X: the [M, K] row-major matrix, or (xf & 1) a flat fragment-major buffer of rows rows
static std::pair<int64_t, int64_t> sk_x_shape(const at::Tensor& x, const at::Tensor& wf, int64_t N, int64_t xf,
                                              int64_t rows) {
  need(x, at::kBFloat16, "x");
  need(wf, at::kBFloat16, "wf");
  TORCH_CHECK(N > 0 && wf.numel() % N == 0, "gemm_sk: weight numel not a multiple of N");
  if (xf & 1) {
    const int64_t K = wf.numel() / N;
    TORCH_CHECK(rows > 0 && x.is_contiguous() && x.numel() >= (rows + 15) / 16 * 16 * K,
                "gemm_sk: fragment-major x needs rows and ceil(rows / 16) * 16 * K elements");
    return {rows, K};
  }
  TORCH_CHECK(x.dim() == 2 && x.stride(1) == 1, "x must be a row-major matrix");
  TORCH_CHECK(wf.numel() == N * x.size(1), "weight numel mismatch");
  return {x.size(0), x.size(1)};
}

int64_t gemm_sk(const at::Tensor& x, const at::Tensor& wf, int64_t N, at::Tensor& out, int64_t epi, at::Tensor& ws,
                at::Tensor& tickets, int64_t ncu, int64_t min_share, int64_t cfg, int64_t xf, int64_t rows) {
  need(ws, at::kFloat, "ws");
  need(tickets, at::kInt, "tickets");
  TORCH_CHECK(xf >= 0 && xf <= 3 && (!(xf & 2) || (epi == 2 && N % 64 == 0)),
              "gemm_sk: xf (+2 only with the SiLU epilogue and N / 2 % 32 == 0)");
  const auto mk = sk_x_shape(x, wf, N, xf, rows);
  const int M = (int)mk.first, K = (int)mk.second;
  TORCH_CHECK(M > 0, "gemm_sk: no rows");
  TORCH_CHECK(ncu >= 8 && ncu <= 1024, "gemm_sk: ncu out of range");
  TORCH_CHECK(ws.numel() * 4 >= lsa_gemm_sk_ws_bytes((int)ncu) && tickets.numel() >= lsa_gemm_sk_tickets((int)ncu),
              "gemm_sk: workspace too small");
  TORCH_CHECK(epi >= 0 && epi <= 3, "gemm_sk: epi");
  if (epi == 1 || epi == 3) {
    need(out, at::kFloat, "out");
    TORCH_CHECK(out.numel() >= (int64_t)M * N, "f32 out too small");
  } else {
    need(out, at::kBFloat16, "out");
    TORCH_CHECK(out.numel() >= (int64_t)((xf & 2) ? (M + 15) / 16 * 16 : M) * (epi == 2 ? N / 2 : N),
                "bf16 out too small");
  }
  TORCH_CHECK(cfg >= -1 && cfg < 64, "gemm_sk: cfg");
  int grid = 0, used = 0;
  check(lsa_gemm_sk(x.data_ptr(), (xf & 1) ? 0 : (int)x.stride(0), M, K, wf.data_ptr(), N, out.data_ptr(), (int)epi,
                    ws.data_ptr<float>(), tickets.data_ptr<int>(), (int)ncu, (int)min_share, (int)cfg, (int)xf, &grid,
                    &used, cur_stream()),
        "gemm_sk");
  return (int64_t)grid * 16 + used;
}

// the prefill qkv projection with RoPE and the paged bf16 KV-cache append in its epilogue (gemm_tile256.hip
// EPI_ROPE): q_out [T, H, 128], kc / vc [blocks, Hkv, 64, 128] bf16, pos / tok_seq [T] int32, block_tables
// [seqs, max_blocks] int32, cos / sin [max_pos, 64] f32.  Returns grid * 16 + the configuration used.
int64_t gemm_sk_rope(const at::Tensor& x, const at::Tensor& wf, at::Tensor& ws, at::Tensor& tickets, int64_t ncu,
                     int64_t min_share, int64_t cfg, const at::Tensor& pos, const c10::optional<at::Tensor>& tok_seq,
                     const at::Tensor& block_tables, const at::Tensor& cos_t, const at::Tensor& sin_t,
                     at::Tensor& q_out, at::Tensor& kc, at::Tensor& vc, int64_t H, int64_t Hkv, int64_t xf,
                     int64_t rows) {
  need(ws, at::kFloat, "ws");
  need(tickets, at::kInt, "tickets");
  need(pos, at::kInt, "pos");
  need(block_tables, at::kInt, "block_tables");
  need(cos_t, at::kFloat, "cos_t");
  need(sin_t, at::kFloat, "sin_t");
  need(q_out, at::kBFloat16, "q_out");
  need(kc, at::kBFloat16, "kc");
  need(vc, at::kBFloat16, "vc");
  TORCH_CHECK(xf == 0 || xf == 1, "gemm_sk_rope: xf 0 | 1");
  const int64_t N = (H + 2 * Hkv) * 128;
  TORCH_CHECK(H > 0 && Hkv > 0, "gemm_sk_rope: heads");
  const auto mk = sk_x_shape(x, wf, N, xf, rows);
  const int64_t M = mk.first, K = mk.second;
  TORCH_CHECK(pos.numel() >= M && q_out.is_contiguous() && q_out.numel() >= M * H * 128, "gemm_sk_rope: q_out / pos");
  TORCH_CHECK(kc.dim() == 4 && kc.size(1) == Hkv && kc.size(2) == 64 && kc.size(3) == 128 && kc.sizes() == vc.sizes() &&
                  kc.is_contiguous() && vc.is_contiguous(), "gemm_sk_rope: cache [blocks, Hkv, 64, 128]");
  TORCH_CHECK(block_tables.dim() == 2 && block_tables.is_contiguous(), "gemm_sk_rope: block_tables [seqs, max_blocks]");
  TORCH_CHECK(cos_t.dim() == 2 && cos_t.size(1) == 64 && cos_t.sizes() == sin_t.sizes(), "gemm_sk_rope: cos / sin");
  if (tok_seq.has_value()) {
    need(*tok_seq, at::kInt, "tok_seq");
    TORCH_CHECK(tok_seq->numel() >= M, "gemm_sk_rope: tok_seq");
  }
  TORCH_CHECK(ncu >= 8 && ncu <= 1024 && ws.numel() * 4 >= lsa_gemm_sk_ws_bytes((int)ncu) &&
                  tickets.numel() >= lsa_gemm_sk_tickets((int)ncu), "gemm_sk_rope: workspace too small");
  int grid = 0, used = 0;
  check(lsa_gemm_sk_rope(x.data_ptr(), xf ? 0 : (int)x.stride(0), (int)M, (int)K, wf.data_ptr(), (int)N, ws.data_ptr<float>(),
                         tickets.data_ptr<int>(), (int)ncu, (int)min_share, (int)cfg, pos.data_ptr<int>(),
                         ptr<int>(tok_seq), block_tables.data_ptr<int>(), (int)block_tables.size(1),
                         cos_t.data_ptr<float>(), sin_t.data_ptr<float>(), q_out.data_ptr(), kc.data_ptr(),
                         vc.data_ptr(), (int)H, (int)Hkv, (int)xf, &grid, &used, cur_stream()),
        "gemm_sk_rope");
  return (int64_t)grid * 16 + used;
}

void fp8_gemm(const at::Tensor& x, const at::Tensor& wq, const at::Tensor& wscale, int64_t N, at::Tensor& out,
              int64_t epi, int64_t nb, int64_t splitk, int64_t waves, int64_t depth,
              const c10::optional<at::Tensor>& rowss, double eps,
              const c10::optional<at::Tensor>& h, const c10::optional<at::Tensor>& xout, int64_t xmt,
              const c10::optional<at::Tensor>& ss_out, const c10::optional<at::Tensor>& tickets) {
  need(x, at::kBFloat16, "x");
  TORCH_CHECK(on_dev(wq) && wq.element_size() == 1, "wq must be a 1-byte GPU tensor");
  need(wscale, at::kFloat, "wscale");
  TORCH_CHECK(x.dim() == 2 && x.stride(1) == 1, "x must be a row-major matrix");
  const int M = x.size(0), K = x.size(1);
  TORCH_CHECK(wq.numel() == N * K, "fp8 weight numel mismatch");
  const EpiOpts eo = epi_opts(epi, M, N, K, rowss, eps, h, xout, xmt, ss_out, tickets, N / 16);
  lsa_fp8_gemm_knobs((int)waves, (int)depth);
  check(lsa_fp8_gemm_ex(x.data_ptr(), x.stride(0), M, K, wq.data_ptr(), wscale.data_ptr<float>(), N, out.data_ptr(),
                        epi, nb, splitk, 0, eo.on ? &eo.e : nullptr, cur_stream()),
        "fp8_gemm");
}

// MXFP4 weights (kernels/gemm_fp4.hip, ops.pack_mxfp4): wq [N/16, K/128, 64, 16] e2m1 nibbles, sw [N/16, KB4, 64, 4]
// E8M0 block scales (KB4 = ceil(K / 512))
void check_fp4(const at::Tensor& wq, const at::Tensor& sw, int64_t N, int64_t K) {
  TORCH_CHECK(N % 16 == 0 && K % 128 == 0, "mxfp4: N % 16 == 0, K % 128 == 0");
  TORCH_CHECK(on_dev(wq) && wq.element_size() == 1 && wq.is_contiguous() && wq.numel() == N * K / 2,
              "wq must be N*K/2 contiguous e2m1 bytes");
  TORCH_CHECK(on_dev(sw) && sw.element_size() == 1 && sw.is_contiguous() && sw.numel() == (N / 16) * ((K / 128 + 3) / 4) * 256,
              "sw must be the [N/16, ceil(K/512), 64, 4] E8M0 scale bytes");
}

void fp4_gemm(const at::Tensor& x, const at::Tensor& wq, const at::Tensor& sw, int64_t N, at::Tensor& out, int64_t epi,
              int64_t nb, int64_t splitk, int64_t waves, const c10::optional<at::Tensor>& rowss, double eps,
              const c10::optional<at::Tensor>& h, const c10::optional<at::Tensor>& xout, int64_t xmt,
              const c10::optional<at::Tensor>& ss_out, const c10::optional<at::Tensor>& tickets) {
  need(x, at::kBFloat16, "x");
  TORCH_CHECK(x.dim() == 2 && x.stride(1) == 1, "x must be a row-major matrix");
  const int64_t M = x.size(0), K = x.size(1);
  TORCH_CHECK(M >= 1 && M <= 64, "fp4_gemm: decode rows 1..64 (prefill dequantises, fp4_dequant)");
  check_fp4(wq, sw, N, K);
  check_out(epi, out, splitk, M, N, 0);
  const EpiOpts eo = epi_opts(epi, M, N, K, rowss, eps, h, xout, xmt, ss_out, tickets, N / 16);
  check(lsa_fp4_gemm_ex(x.data_ptr(), x.stride(0), M, K, wq.data_ptr(), sw.data_ptr(), N, out.data_ptr(), epi, nb, splitk,
                        waves, 0, eo.on ? &eo.e : nullptr, cur_stream()),
        "fp4_gemm");
}

void fp4_gemm_xf(const at::Tensor& xf, int64_t M, int64_t K, const at::Tensor& wq, const at::Tensor& sw, int64_t N,
                 at::Tensor& out, int64_t epi, int64_t nb, int64_t splitk, int64_t waves,
                 const c10::optional<at::Tensor>& rowss, double eps, const c10::optional<at::Tensor>& h,
                 const c10::optional<at::Tensor>& xout, int64_t xmt, const c10::optional<at::Tensor>& ss_out,
                 const c10::optional<at::Tensor>& tickets) {
  need(xf, at::kBFloat16, "xf");
  TORCH_CHECK(M >= 1 && M <= 64, "fp4_gemm_xf: M in 1..64");
  check_fp4(wq, sw, N, K);
  const int64_t mt = M <= 16 ? 1 : (M <= 32 ? 2 : 4);
  TORCH_CHECK(xf.is_contiguous() && xf.numel() >= mt * 16 * K, "xf too small");
  check_out(epi, out, splitk, M, N, mt);
  const EpiOpts eo = epi_opts(epi, M, N, K, rowss, eps, h, xout, xmt, ss_out, tickets, N / 16);
  check(lsa_fp4_gemm_ex(xf.data_ptr(), K, M, K, wq.data_ptr(), sw.data_ptr(), N, out.data_ptr(), epi, nb, splitk, waves,
                        1, eo.on ? &eo.e : nullptr, cur_stream()),
        "fp4_gemm_xf");
}

void fp4_dequant(const at::Tensor& wq, const at::Tensor& sw, int64_t N, int64_t K, at::Tensor& wf) {
  check_fp4(wq, sw, N, K);
  need(wf, at::kBFloat16, "wf");
  TORCH_CHECK(wf.is_contiguous() && wf.numel() >= N * K, "fp4_dequant: output too small");
  check(lsa_fp4_dequant(wq.data_ptr(), sw.data_ptr(), N, K, wf.data_ptr(), cur_stream()), "fp4_dequant");
}

// GGUF Q4_0 weights (kernels/gemm_q4.hip, ops.pack_q4_0): wq [N/16, K/128, 64, 16] codes, dw [N/16, ceil(K/256), 64, 2]
// f16 block scales.  The refusals of lsa_q4_gemm_ex (shape, row count, split-K with a non-f32 epilogue) are left to it:
// a call it would refuse goes straight to it, it returns its code before any launch or memory access, and the code
// surfaces as the exception.  The checks here are what it cannot see: dtypes, devices and buffer sizes.
bool q4_launcher_refuses(int64_t M, int64_t N, int64_t K, int64_t epi, int64_t splitk) {
  return N <= 0 || K <= 0 || N % 16 != 0 || K % 128 != 0 || M <= 0 || M > 64 || (epi != 1 && splitk > 1);
}

void check_q4(const at::Tensor& wq, const at::Tensor& dw, int64_t N, int64_t K) {
  TORCH_CHECK(N > 0 && K > 0 && N % 16 == 0 && K % 128 == 0, "q4_0: N % 16 == 0, K % 128 == 0");
  TORCH_CHECK(on_dev(wq) && wq.element_size() == 1 && wq.is_contiguous() && wq.numel() == N * K / 2,
              "wq must be N*K/2 contiguous Q4_0 code bytes");
  TORCH_CHECK(on_dev(dw) && dw.is_contiguous() &&
                  dw.numel() * dw.element_size() == (N / 16) * ((K / 128 + 1) / 2) * 256,
              "dw must be the [N/16, ceil(K/256), 64, 2] f16 block scales");
}

void q4_gemm(const at::Tensor& x, const at::Tensor& wq, const at::Tensor& dw, int64_t N, at::Tensor& out, int64_t epi,
             int64_t nb, int64_t splitk, int64_t waves, const c10::optional<at::Tensor>& rowss, double eps) {
  need(x, at::kBFloat16, "x");
  TORCH_CHECK(x.dim() == 2 && x.stride(1) == 1, "x must be a row-major matrix");
  const int64_t M = x.size(0), K = x.size(1);
  TORCH_CHECK(epi >= 0 && epi <= 2, "q4_gemm: epilogue bf16 | f32 | silu");
  if (q4_launcher_refuses(M, N, K, epi, splitk))
    check(lsa_q4_gemm_ex(nullptr, 0, M, K, nullptr, nullptr, N, nullptr, epi, nb, splitk, waves, 0, nullptr, cur_stream()),
          "q4_gemm");
  check_q4(wq, dw, N, K);
  check_out(epi, out, splitk, M, N, 0);
  const EpiOpts eo = epi_opts(epi, M, N, K, rowss, eps, c10::nullopt, c10::nullopt, 0, c10::nullopt, c10::nullopt, N / 16);
  check(lsa_q4_gemm_ex(x.data_ptr(), x.stride(0), M, K, wq.data_ptr(), dw.data_ptr(), N, out.data_ptr(), epi, nb, splitk,
                       waves, 0, eo.on ? &eo.e : nullptr, cur_stream()),
        "q4_gemm");
}

void q4_gemm_xf(const at::Tensor& xf, int64_t M, int64_t K, const at::Tensor& wq, const at::Tensor& dw, int64_t N,
                at::Tensor& out, int64_t epi, int64_t nb, int64_t splitk, int64_t waves,
                const c10::optional<at::Tensor>& rowss, double eps) {
  need(xf, at::kBFloat16, "xf");
  TORCH_CHECK(epi >= 0 && epi <= 2, "q4_gemm_xf: epilogue bf16 | f32 | silu");
  if (q4_launcher_refuses(M, N, K, epi, splitk))
    check(lsa_q4_gemm_ex(nullptr, 0, M, K, nullptr, nullptr, N, nullptr, epi, nb, splitk, waves, 1, nullptr, cur_stream()),
          "q4_gemm_xf");
  check_q4(wq, dw, N, K);
  const int64_t mt = M <= 16 ? 1 : (M <= 32 ? 2 : 4);
  TORCH_CHECK(xf.is_contiguous() && xf.numel() >= mt * 16 * K, "xf too small");
  check_out(epi, out, splitk, M, N, mt);
  const EpiOpts eo = epi_opts(epi, M, N, K, rowss, eps, c10::nullopt, c10::nullopt, 0, c10::nullopt, c10::nullopt, N / 16);
  check(lsa_q4_gemm_ex(xf.data_ptr(), K, M, K, wq.data_ptr(), dw.data_ptr(), N, out.data_ptr(), epi, nb, splitk, waves,
                       1, eo.on ? &eo.e : nullptr, cur_stream()),
        "q4_gemm_xf");
}

void q4_dequant(const at::Tensor& wq, const at::Tensor& dw, int64_t N, int64_t K, at::Tensor& wf) {
  check_q4(wq, dw, N, K);
  need(wf, at::kBFloat16, "wf");
  TORCH_CHECK(wf.is_contiguous() && wf.numel() >= N * K, "q4_dequant: output too small");
  check(lsa_q4_dequant(wq.data_ptr(), dw.data_ptr(), N, K, wf.data_ptr(), cur_stream()), "q4_dequant");
}

void add_rmsnorm(at::Tensor& h, const c10::optional<at::Tensor>& parts, int64_t nparts, int64_t part_stride,
                 const c10::optional<at::Tensor>& ids, const c10::optional<at::Tensor>& emb,
                 const c10::optional<at::Tensor>& row_idx, bool write_h, const at::Tensor& w, double eps,
                 const c10::optional<at::Tensor>& xn, int64_t rows, int64_t xf_mt, const c10::optional<at::Tensor>& ss_out,
                 int64_t ss_ld, int64_t ss_nzero, const c10::optional<at::Tensor>& x8,
                 const c10::optional<at::Tensor>& sx8) {
  need(h, at::kFloat, "h");
  need(w, at::kBFloat16, "w");
  if (xn.has_value()) need(*xn, at::kBFloat16, "xn");
  if (x8.has_value()) {
    TORCH_CHECK(on_dev(*x8) && x8->element_size() == 1 && x8->numel() >= xf_mt * 16 * w.numel(), "x8 too small");
    TORCH_CHECK(sx8.has_value() && sx8->scalar_type() == at::kFloat && sx8->numel() >= rows, "x8 needs sx8 [rows] f32");
  }
  const int D = w.numel();
  if (ss_out.has_value()) {
    need(*ss_out, at::kLong, "ss_out");
    TORCH_CHECK(ss_out->numel() >= (ss_nzero + 1) * ss_ld && ss_ld >= rows, "ss_out too small");
  }
  check(lsa_add_rmsnorm(h.data_ptr<float>(), ptr<const float>(parts), parts.has_value() ? nparts : 0, part_stride,
                        ptr<const int>(ids), ptr<const void>(emb), ptr<const int>(row_idx), write_h ? 1 : 0,
                        w.data_ptr(), (float)eps, xn.has_value() ? xn->data_ptr() : nullptr, rows, D, xf_mt,
                        ss_out.has_value() ? reinterpret_cast<long long*>(ss_out->data_ptr<int64_t>()) : nullptr, (int)ss_ld,
                        (int)ss_nzero, x8.has_value() ? x8->data_ptr() : nullptr,
                        sx8.has_value() ? sx8->data_ptr<float>() : nullptr, cur_stream()),
        "add_rmsnorm");
}

// y: bf16 [M, 2F] (gate/up interleaved per 16 columns, the vendor prefill GEMM's output) -> out bf16 [M, F]
void silu_bf16(const at::Tensor& y, at::Tensor& out) {
  need(y, at::kBFloat16, "y");
  need(out, at::kBFloat16, "out");
  TORCH_CHECK(y.dim() == 2 && y.is_contiguous() && y.size(1) % 32 == 0, "silu_bf16: y [M, 2F] contiguous");
  const int M = y.size(0), F = y.size(1) / 2;
  TORCH_CHECK(out.is_contiguous() && out.numel() >= (int64_t)M * F, "silu_bf16: out too small");
  check(lsa_silu_bf16(y.data_ptr(), M, F, out.data_ptr(), cur_stream()), "silu_bf16");
}

// Infinity-Cache warm-up of up to four tensors (the first bytes[k] bytes of each; -1 = all of it)
void prefetch(const std::vector<at::Tensor>& ts, const std::vector<int64_t>& bytes, int64_t wgs) {
  TORCH_CHECK(!ts.empty() && ts.size() <= 4 && bytes.size() == ts.size(), "prefetch: 1-4 tensors, one byte count each");
  const void* ptrs[4];
  long nb[4];
  for (size_t k = 0; k < ts.size(); ++k) {
    TORCH_CHECK(on_dev(ts[k]) && ts[k].is_contiguous(), "prefetch: contiguous GPU tensors");
    const int64_t all = ts[k].numel() * ts[k].element_size();
    ptrs[k] = ts[k].data_ptr();
    nb[k] = (long)(bytes[k] < 0 || bytes[k] > all ? all : bytes[k]);
  }
  check(lsa_prefetch(ptrs, nb, (int)ts.size(), (int)wgs, cur_stream()), "prefetch");
}

// wide raw residual add of the folded-norm decode step: h += sum parts; xn = bf16(h); ss_out[m] += sum h^2 (Q24)
void res_add_ss(at::Tensor& h, const c10::optional<at::Tensor>& parts, int64_t nparts, int64_t part_stride,
                at::Tensor& xn, int64_t rows, int64_t D, int64_t xf_mt, at::Tensor& ss_out) {
  need(h, at::kFloat, "h");
  need(xn, at::kBFloat16, "xn");
  need(ss_out, at::kLong, "ss_out");
  TORCH_CHECK(rows > 0 && D > 0 && D % 8 == 0, "res_add_ss: bad rows / D");
  TORCH_CHECK(h.is_contiguous() && h.numel() >= rows * D, "res_add_ss: h too small");
  TORCH_CHECK(xn.is_contiguous() && xn.numel() >= (xf_mt > 0 ? xf_mt * 16 : rows) * D, "res_add_ss: xn too small");
  TORCH_CHECK(xf_mt <= 0 || (D % 32 == 0 && rows <= 16 * xf_mt), "res_add_ss: xf tiles");
  TORCH_CHECK(ss_out.is_contiguous() && ss_out.numel() >= rows, "res_add_ss: ss_out too small");
  if (parts.has_value() && nparts > 0) {
    need(*parts, at::kFloat, "parts");
    TORCH_CHECK(part_stride >= rows * D && parts->numel() >= (nparts - 1) * part_stride + rows * D,
                "res_add_ss: parts too small");
  }
  check(lsa_res_add_ss(h.data_ptr<float>(), parts.has_value() && nparts > 0 ? parts->data_ptr<float>() : nullptr,
                       parts.has_value() ? (int)nparts : 0, part_stride, xn.data_ptr(), (int)rows, (int)D,
                       (int)(xf_mt > 0 ? xf_mt : 0), reinterpret_cast<long long*>(ss_out.data_ptr<int64_t>()),
                       cur_stream()),
        "res_add_ss");
}

void rope_append(const at::Tensor& qkv, const at::Tensor& pos, const c10::optional<at::Tensor>& tok_seq,
                 const at::Tensor& block_tables, const at::Tensor& cos_t, const at::Tensor& sin_t, at::Tensor& q_out,
                 at::Tensor& kc, at::Tensor& vc, int64_t H, int64_t Hkv, const c10::optional<at::Tensor>& ks,
                 const c10::optional<at::Tensor>& vs) {
  need(pos, at::kInt, "pos");
  check_cache(kc, vc, ks, vs);
  need(block_tables, at::kInt, "block_tables");
  need(cos_t, at::kFloat, "cos");
  need(sin_t, at::kFloat, "sin");
  need(q_out, at::kBFloat16, "q_out");
  // qkv: bf16 [T, n] or f32 split-K slabs [S, T, n]
  const bool parts = qkv.scalar_type() == at::kFloat;
  TORCH_CHECK(parts || qkv.scalar_type() == at::kBFloat16, "qkv must be bf16 or f32 slabs");
  const int T = parts ? qkv.size(1) : qkv.size(0);
  TORCH_CHECK(qkv.size(qkv.dim() - 1) == (H + 2 * Hkv) * 128 && pos.numel() >= T && q_out.numel() >= (int64_t)T * H * 128,
              "rope_append: qkv [.., T, (H + 2 Hkv) * 128], pos [T], q_out [T, H, 128]");
  TORCH_CHECK(cos_t.size(0) >= block_tables.size(1) * 64 && sin_t.size(0) >= block_tables.size(1) * 64,
              "rope tables have fewer rows than the block tables address (", block_tables.size(1) * 64, ")");
  check(lsa_rope_append(parts ? nullptr : qkv.data_ptr(), parts ? qkv.data_ptr<float>() : nullptr,
                        parts ? qkv.size(0) : 0, parts ? qkv.stride(0) : 0, pos.data_ptr<int>(), ptr<const int>(tok_seq), block_tables.data_ptr<int>(),
                        block_tables.size(1), cos_t.data_ptr<float>(), sin_t.data_ptr<float>(), q_out.data_ptr(),
                        kc.data_ptr(), vc.data_ptr(), ptr<float>(ks), ptr<float>(vs), T, H, Hkv, cur_stream()),
        "rope_append");
}

void silu_mul(const at::Tensor& g, const at::Tensor& u, at::Tensor& o) {
  need(g, at::kBFloat16, "g");
  need(u, at::kBFloat16, "u");
  need(o, at::kBFloat16, "o");
  TORCH_CHECK(u.numel() == g.numel() && o.numel() >= g.numel() && g.is_contiguous() && u.is_contiguous() &&
                  o.is_contiguous(), "silu_mul: contiguous g, u of equal size and o at least as large");
  check(lsa_silu_mul(g.data_ptr(), u.data_ptr(), o.data_ptr(), g.numel(), cur_stream()), "silu_mul");
}

extern "C" int lsa_attn_set_stamps(void* p);
void attn_set_stamps(const c10::optional<at::Tensor>& st) {
  if (st.has_value()) TORCH_CHECK(on_dev(*st) && st->element_size() == 8, "stamps: int64 GPU tensor");
  check(lsa_attn_set_stamps(st.has_value() ? st->data_ptr() : nullptr), "attn_set_stamps");
}

// diagnostic stamps of the stream-K prefill GEMM (kernels/gemm_tile256.hip g_sk_stamps): [grid][8] int64, sized by the
// caller for the largest grid it launches (<= 2 x CUs)
extern "C" int lsa_sk_set_stamps(unsigned long long* p);
void sk_set_stamps(const c10::optional<at::Tensor>& st) {
  if (st.has_value()) TORCH_CHECK(on_dev(*st) && st->element_size() == 8 && st->numel() >= 2048 * 8,
                                  "stamps: int64 GPU tensor of >= 2048 x 8");
  check(lsa_sk_set_stamps(st.has_value() ? reinterpret_cast<unsigned long long*>(st->data_ptr()) : nullptr),
        "sk_set_stamps");
}

// diagnostic cycle stamps of the 32-row prefill attention (kernels/attention_prefill32.hip g_p32_stamps): the caller
// sizes the buffer for the plan it launches, [nwork * H * NG * 4][8] int64
extern "C" int lsa_p32_set_stamps(void* p);
void attn_prefill_set_stamps(const c10::optional<at::Tensor>& st) {
  if (st.has_value()) TORCH_CHECK(on_dev(*st) && st->element_size() == 8 && st->is_contiguous(), "stamps: int64 GPU tensor");
  check(lsa_p32_set_stamps(st.has_value() ? st->data_ptr() : nullptr), "attn_prefill_set_stamps");
}

void attn_decode(const at::Tensor& q, const at::Tensor& kc, const at::Tensor& vc, const at::Tensor& block_tables,
                 const at::Tensor& pos, int64_t H, int64_t Hkv, double scale, int64_t chunk_blocks, int64_t nsplit,
                 at::Tensor& out, at::Tensor& opart, at::Tensor& mlpart, at::Tensor& counters, int64_t xf_mt,
                 const c10::optional<at::Tensor>& qkv_parts, const c10::optional<at::Tensor>& cos_t,
                 const c10::optional<at::Tensor>& sin_t, int64_t unsplit_max, const c10::optional<at::Tensor>& ks,
                 const c10::optional<at::Tensor>& vs, const c10::optional<at::Tensor>& out_s8 = c10::nullopt,
                 const c10::optional<at::Tensor>& rowss = c10::nullopt, double eps = 1e-5, int64_t hidden = 0) {
  need(q, at::kBFloat16, "q");
  if (rowss.has_value()) {  // residual-reduce decode step: the slabs are the projection of un-normalised rows
    TORCH_CHECK(qkv_parts.has_value() && hidden > 0, "attn_decode rowss: needs qkv_parts and the hidden size");
    need(*rowss, at::kLong, "rowss");
    TORCH_CHECK(rowss->numel() >= pos.size(0), "attn_decode: rowss too small");
  }
  check_cache(kc, vc, ks, vs);
  need(pos, at::kInt, "pos");
  need(block_tables, at::kInt, "block_tables");
  const int B = pos.size(0);
  TORCH_CHECK(block_tables.dim() == 2 && block_tables.size(0) >= B && block_tables.is_contiguous(),
              "block_tables [>= B, max_blocks]");
  TORCH_CHECK(H > 0 && Hkv > 0 && H % Hkv == 0 && kc.size(1) == Hkv, "heads: H % Hkv == 0, cache has Hkv heads");
  if (out_s8.has_value()) {  // e4m3 output (xf8 layout) + E8M0 per (row, head): the W8A8 / W4A8 o projection's input
    TORCH_CHECK(xf_mt > 0 && on_dev(out) && out.element_size() == 1 && out.numel() >= xf_mt * 16 * H * 128,
                "attn_decode: e4m3 out needs xf_mt and xf_mt * 16 * H * 128 bytes");
    TORCH_CHECK(on_dev(*out_s8) && out_s8->element_size() == 1 && out_s8->numel() >= xf_mt * 64 * H,
                "attn_decode: out_s8 too small");
  } else {
    need(out, at::kBFloat16, "out");
    TORCH_CHECK(out.numel() >= (xf_mt ? xf_mt * 16 : B) * H * 128, "attn_decode out too small");
  }
  need(opart, at::kFloat, "opart");
  need(mlpart, at::kFloat, "mlpart");
  need(counters, at::kInt, "counters");
  TORCH_CHECK(opart.numel() >= (int64_t)B * H * nsplit * 128 && mlpart.numel() >= (int64_t)B * H * nsplit * 2 &&
                  counters.numel() >= (int64_t)B * Hkv,
              "attn_decode workspace too small");
  TORCH_CHECK(opart.numel() * 4 < 0x7fffffffLL, "opart must stay below 2 GiB (buffer descriptor range)");
  if (qkv_parts.has_value()) {  // fused RoPE + KV append from the QKV projection's f32 split-K slabs
    need(*qkv_parts, at::kFloat, "qkv_parts");
    TORCH_CHECK(qkv_parts->dim() == 3 && qkv_parts->size(1) >= B && qkv_parts->size(2) == (H + 2 * Hkv) * 128 &&
                    qkv_parts->stride(1) == qkv_parts->size(2) && qkv_parts->stride(2) == 1,
                "qkv_parts must be [S, B, (H + 2 Hkv) * 128] row-major slabs");
    TORCH_CHECK(cos_t.has_value() && sin_t.has_value(), "fused rope needs cos/sin tables");
    need(*cos_t, at::kFloat, "cos");
    need(*sin_t, at::kFloat, "sin");
    // positions come from the device (no host read); every position the block tables address needs a row
    TORCH_CHECK(cos_t->size(0) >= block_tables.size(1) * 64 && sin_t->size(0) >= block_tables.size(1) * 64,
                "rope tables have fewer rows than the block tables address (", block_tables.size(1) * 64, ")");
  }
  check(lsa_attn_decode(q.data_ptr(), kc.data_ptr(), vc.data_ptr(), block_tables.data_ptr<int>(),
                        block_tables.size(1), pos.data_ptr<int>(), B, H, Hkv, (float)scale, chunk_blocks, nsplit,
                        (int)unsplit_max, out.data_ptr(), opart.data_ptr<float>(), mlpart.data_ptr<float>(), counters.data_ptr<int>(), xf_mt,
                        ptr<const float>(qkv_parts), qkv_parts.has_value() ? qkv_parts->size(0) : 0,
                        qkv_parts.has_value() ? qkv_parts->stride(0) : 0, ptr<const float>(cos_t),
                        ptr<const float>(sin_t), ptr<const float>(ks), ptr<const float>(vs),
                        out_s8.has_value() ? out_s8->data_ptr() : nullptr,
                        rowss.has_value() ? reinterpret_cast<const long long*>(rowss->data_ptr<int64_t>()) : nullptr,
                        rowss.has_value() ? 1.0f / (float)hidden : 0.f, (float)eps, cur_stream()),
        "attn_decode");
}

// fp8 cache blocks of a prefill batch -> compact bf16 scratch [nseq * mb, Hkv, 64, 128] (kernels/kv8.hip)
void kv8_dequant(const at::Tensor& kc, const at::Tensor& vc, const at::Tensor& ks, const at::Tensor& vs,
                 const at::Tensor& block_tables, const at::Tensor& ctx_lens, int64_t mb, at::Tensor& ko, at::Tensor& vo) {
  check_cache(kc, vc, ks, vs);
  need(block_tables, at::kInt, "block_tables");
  need(ctx_lens, at::kInt, "ctx_lens");
  need(ko, at::kBFloat16, "ko");
  need(vo, at::kBFloat16, "vo");
  const int64_t nseq = ctx_lens.numel(), Hkv = kc.size(1);
  TORCH_CHECK(block_tables.dim() == 2 && block_tables.size(0) >= nseq && block_tables.is_contiguous(),
              "block_tables must be a contiguous [nseq, max_blocks] table");
  TORCH_CHECK(mb <= block_tables.size(1), "mb exceeds the block table width");
  TORCH_CHECK(ko.numel() >= nseq * mb * Hkv * 64 * 128 && vo.numel() >= nseq * mb * Hkv * 64 * 128, "kv8 scratch too small");
  check(lsa_kv8_dequant(kc.data_ptr(), vc.data_ptr(), ks.data_ptr<float>(), vs.data_ptr<float>(),
                        block_tables.data_ptr<int>(), block_tables.size(1), ctx_lens.data_ptr<int>(), nseq, Hkv, mb,
                        ko.data_ptr(), vo.data_ptr(), cur_stream()),
        "kv8_dequant");
}

// prefix cache: copy whole KV blocks inside the arena kv [L, 2, NB, Hkv, 64, 128] (bf16, or e4m3 bytes with
// scale [L, 2, NB, Hkv, 64] f32) for every (src, dst) row of pairs [n, 2] int32 (kernels/kv_copy.hip).  The ids
// are validated on the host before they are uploaded (ops.kv_copy_blocks).
void kv_copy_blocks(at::Tensor& kv, const c10::optional<at::Tensor>& scale, const at::Tensor& pairs) {
  need(kv, scale.has_value() ? at::kByte : at::kBFloat16, "kv");
  TORCH_CHECK(kv.dim() == 6 && kv.size(1) == 2 && kv.size(2) >= 2 && kv.size(4) == 64 && kv.size(5) == 128 &&
                  kv.is_contiguous(), "kv must be a contiguous [L, 2, NB, Hkv, 64, 128] arena");
  if (scale.has_value()) {
    need(*scale, at::kFloat, "kv_scale");
    TORCH_CHECK(scale->dim() == 5 && scale->is_contiguous() && scale->sizes() == kv.sizes().slice(0, 5),
                "kv_scale must be a contiguous [L, 2, NB, Hkv, 64] tensor");
  }
  need(pairs, at::kInt, "pairs");
  TORCH_CHECK(pairs.dim() == 2 && pairs.size(1) == 2 && pairs.is_contiguous(), "pairs must be a contiguous [n, 2] tensor");
  const int64_t L = kv.size(0), NB = kv.size(2), Hkv = kv.size(3);
  TORCH_CHECK(NB <= INT32_MAX && pairs.size(0) <= 65535 && 2 * L <= 65535, "kv_copy_blocks: arena or pair list too large");
  check(lsa_kv_copy_blocks(kv.data_ptr(), scale.has_value() ? scale->data_ptr() : nullptr, pairs.data_ptr<int>(),
                           (int)pairs.size(0), (int)(2 * L), (int)NB, Hkv * 64 * 128 * (int64_t)kv.element_size(),
                           scale.has_value() ? Hkv * 64 * 4 : 0, cur_stream()),
        "kv_copy_blocks");
}

// context shift: move rows between blocks of the bf16 arena kv [L, 2, NB, Hkv, 64, 128] and rotate the K rows by
// -delta with the RoPE tables cos / sin [rows, 64] f32, for every (src, dst, row_lo, row_hi, delta) row of moves
// [n, 5] int32 (kernels/kv_shift.hip).  The moves are validated on the host before they are uploaded (ops.kv_shift).
void kv_shift(at::Tensor& kv, const at::Tensor& moves, const at::Tensor& cos, const at::Tensor& sin) {
  need(kv, at::kBFloat16, "kv");
  TORCH_CHECK(kv.dim() == 6 && kv.size(1) == 2 && kv.size(2) >= 2 && kv.size(4) == 64 && kv.size(5) == 128 &&
                  kv.is_contiguous(), "kv must be a contiguous [L, 2, NB, Hkv, 64, 128] arena");
  need(moves, at::kInt, "moves");
  TORCH_CHECK(moves.dim() == 2 && moves.size(1) == 5 && moves.is_contiguous(), "moves must be a contiguous [n, 5] tensor");
  need(cos, at::kFloat, "cos");
  need(sin, at::kFloat, "sin");
  TORCH_CHECK(cos.dim() == 2 && cos.size(1) == 64 && cos.is_contiguous() && sin.is_contiguous() &&
                  sin.sizes() == cos.sizes() && cos.size(0) >= 1, "cos / sin must be contiguous [rows, 64] tables");
  const int64_t L = kv.size(0), NB = kv.size(2), Hkv = kv.size(3);
  TORCH_CHECK(NB <= INT32_MAX && cos.size(0) <= INT32_MAX && moves.size(0) <= 65535 && L <= 65535 && 4 * Hkv <= 65535,
              "kv_shift: arena, tables or move list too large");
  check(lsa_kv_shift(kv.data_ptr(), moves.data_ptr<int>(), (int)moves.size(0), (int)L, (int)NB, (int)Hkv,
                     cos.data_ptr<float>(), sin.data_ptr<float>(), (int)cos.size(0), cur_stream()),
        "kv_shift");
}

// context shift on the fp8 cache: kv the e4m3 arena [L, 2, NB, Hkv, 64, 128] (uint8, tiles in token-pair order),
// kv_scale its f32 row scales [L, 2, NB, Hkv, 64]; rotated K rows are dequantised, rotated and quantised again with a
// new scale, everything else is copied with its scale (kernels/kv_shift.hip).  The moves are validated on the host
// before they are uploaded (ops.kv_shift8).
void kv_shift8(at::Tensor& kv, at::Tensor& kv_scale, const at::Tensor& moves, const at::Tensor& cos,
               const at::Tensor& sin) {
  need(kv, at::kByte, "kv");
  TORCH_CHECK(kv.dim() == 6 && kv.size(1) == 2 && kv.size(2) >= 2 && kv.size(4) == 64 && kv.size(5) == 128 &&
                  kv.is_contiguous(), "kv must be a contiguous [L, 2, NB, Hkv, 64, 128] arena");
  need(kv_scale, at::kFloat, "kv_scale");
  TORCH_CHECK(kv_scale.dim() == 5 && kv_scale.sizes() == kv.sizes().slice(0, 5) && kv_scale.is_contiguous(),
              "kv_scale must be a contiguous [L, 2, NB, Hkv, 64] tensor");
  need(moves, at::kInt, "moves");
  TORCH_CHECK(moves.dim() == 2 && moves.size(1) == 5 && moves.is_contiguous(), "moves must be a contiguous [n, 5] tensor");
  need(cos, at::kFloat, "cos");
  need(sin, at::kFloat, "sin");
  TORCH_CHECK(cos.dim() == 2 && cos.size(1) == 64 && cos.is_contiguous() && sin.is_contiguous() &&
                  sin.sizes() == cos.sizes() && cos.size(0) >= 1, "cos / sin must be contiguous [rows, 64] tables");
  const int64_t L = kv.size(0), NB = kv.size(2), Hkv = kv.size(3);
  TORCH_CHECK(NB <= INT32_MAX && cos.size(0) <= INT32_MAX && moves.size(0) <= 65535 && L <= 65535 && 2 * Hkv <= 65535,
              "kv_shift8: arena, tables or move list too large");
  check(lsa_kv_shift8(kv.data_ptr(), kv_scale.data_ptr<float>(), moves.data_ptr<int>(), (int)moves.size(0), (int)L,
                      (int)NB, (int)Hkv, cos.data_ptr<float>(), sin.data_ptr<float>(), (int)cos.size(0), cur_stream()),
        "kv_shift8");
}

// Embeddings (kernels/embed.hip): h [T, D] f32 prefill residual rows, parts the optional [np, T, D] f32 split-K slabs
// the final norm would add, tseq [T] / cu [n + 1] the prefill's row -> sequence map and row offsets, meta [5, n] int32
// (emode, estart, eslot, efinal, ecount per sequence).  The values of cu / meta are validated on the host before they
// are uploaded (ops._embed_check); the shapes here.
struct EmbedDims {
  int n, T, D, np;
  long stride;
};

EmbedDims embed_dims(const at::Tensor& h, const c10::optional<at::Tensor>& parts, const at::Tensor& cu,
                     const at::Tensor& meta, const char* what) {
  need(h, at::kFloat, "h");
  need(cu, at::kInt, "cu");
  need(meta, at::kInt, "meta");
  TORCH_CHECK(h.dim() == 2 && h.is_contiguous() && h.size(0) >= 1 && h.size(0) <= INT32_MAX / 2 && h.size(1) >= 4 &&
                  h.size(1) % 4 == 0 && h.size(1) <= (1 << 20), what, ": h must be a contiguous [T, D] tensor, D % 4 == 0");
  TORCH_CHECK(meta.dim() == 2 && meta.size(0) == 5 && meta.size(1) >= 1 && meta.size(1) <= 65535 && meta.is_contiguous(),
              what, ": meta must be a contiguous [5, n] tensor, n <= 65535");
  TORCH_CHECK(cu.dim() == 1 && cu.is_contiguous() && cu.numel() == meta.size(1) + 1, what, ": cu must be [n + 1]");
  EmbedDims d{(int)meta.size(1), (int)h.size(0), (int)h.size(1), 0, 0};
  if (parts.has_value()) {
    need(*parts, at::kFloat, "parts");
    TORCH_CHECK(parts->dim() == 3 && parts->size(0) >= 1 && parts->size(0) <= 64 && parts->size(1) == h.size(0) &&
                    parts->size(2) == h.size(1) && parts->stride(2) == 1 && parts->stride(1) == h.size(1) &&
                    parts->stride(0) >= h.numel(), what, ": parts must be [np, T, D] slabs of contiguous rows");
    d.np = (int)parts->size(0);
    d.stride = (long)parts->stride(0);
  }
  return d;
}

void embed_rowscale(const at::Tensor& h, const c10::optional<at::Tensor>& parts, const at::Tensor& tseq,
                    const at::Tensor& cu, const at::Tensor& meta, double eps, at::Tensor& rs) {
  const EmbedDims d = embed_dims(h, parts, cu, meta, "embed_rowscale");
  need(tseq, at::kInt, "tseq");
  need(rs, at::kFloat, "rs");
  TORCH_CHECK(tseq.dim() == 1 && tseq.is_contiguous() && tseq.numel() == d.T, "embed_rowscale: tseq must be [T]");
  TORCH_CHECK(rs.dim() == 1 && rs.is_contiguous() && rs.numel() >= d.T, "embed_rowscale: rs must hold T rows");
  check(lsa_embed_rowscale(h.data_ptr<float>(), ptr<const float>(parts), d.np, d.stride, tseq.data_ptr<int>(),
                           cu.data_ptr<int>(), meta.data_ptr<int>(), d.n, d.T, d.D, (float)eps, rs.data_ptr<float>(),
                           cur_stream()),
        "embed_rowscale");
}

void embed_pool(const at::Tensor& h, const c10::optional<at::Tensor>& parts, const at::Tensor& cu,
                const at::Tensor& meta, const at::Tensor& rs, const at::Tensor& gamma, at::Tensor& acc) {
  const EmbedDims d = embed_dims(h, parts, cu, meta, "embed_pool");
  need(rs, at::kFloat, "rs");
  need(gamma, at::kBFloat16, "gamma");
  need(acc, at::kFloat, "acc");
  TORCH_CHECK(rs.dim() == 1 && rs.is_contiguous() && rs.numel() >= d.T, "embed_pool: rs must hold T rows");
  TORCH_CHECK(gamma.dim() == 1 && gamma.is_contiguous() && gamma.numel() == d.D, "embed_pool: gamma must be [D]");
  TORCH_CHECK(acc.dim() == 2 && acc.is_contiguous() && acc.size(1) == d.D && acc.size(0) >= 1 &&
                  acc.size(0) <= INT32_MAX, "embed_pool: acc must be a contiguous [slots, D] tensor");
  check(lsa_embed_pool(h.data_ptr<float>(), ptr<const float>(parts), d.np, d.stride, cu.data_ptr<int>(),
                       meta.data_ptr<int>(), d.n, d.T, d.D, rs.data_ptr<float>(), gamma.data_ptr(),
                       acc.data_ptr<float>(), (int)acc.size(0), cur_stream()),
        "embed_pool");
}

void embed_finish(const at::Tensor& meta, const at::Tensor& acc, at::Tensor& out) {
  need(meta, at::kInt, "meta");
  need(acc, at::kFloat, "acc");
  need(out, at::kFloat, "out");
  TORCH_CHECK(meta.dim() == 2 && meta.size(0) == 5 && meta.size(1) >= 1 && meta.size(1) <= INT32_MAX / 8 &&
                  meta.is_contiguous(), "embed_finish: meta must be a contiguous [5, n] tensor");
  TORCH_CHECK(acc.dim() == 2 && acc.is_contiguous() && out.is_contiguous() && out.sizes() == acc.sizes() &&
                  acc.size(0) >= 1 && acc.size(0) <= INT32_MAX && acc.size(1) >= 1 && acc.size(1) <= (1 << 20),
              "embed_finish: acc and out must be contiguous [slots, D] tensors of one shape");
  check(lsa_embed_finish(meta.data_ptr<int>(), (int)meta.size(1), (int)acc.size(1), acc.data_ptr<float>(),
                         out.data_ptr<float>(), (int)acc.size(0), cur_stream()),
        "embed_finish");
}

void attn_prefill(const at::Tensor& q, const at::Tensor& kc, const at::Tensor& vc, const at::Tensor& block_tables,
                  const at::Tensor& cu_q, const at::Tensor& ctx_lens, const at::Tensor& work, int64_t H, int64_t Hkv,
                  double scale, at::Tensor& out, int64_t rows32, int64_t xf_mt) {
  need(q, at::kBFloat16, "q");
  need(work, at::kInt, "work");
  need(cu_q, at::kInt, "cu_q");
  need(ctx_lens, at::kInt, "ctx_lens");
  need(block_tables, at::kInt, "block_tables");
  need(out, at::kBFloat16, "out");
  TORCH_CHECK(q.dim() == 3 && q.size(1) == H && q.size(2) == 128, "q [T, H, 128]");
  // out: [T, H, 128] row-major, or (xf_mt > 0) a flat buffer in the fragment-major layout of xf_mt 16-row tiles (the
  // o projection's stream-K input)
  TORCH_CHECK(xf_mt >= 0 && (xf_mt ? (out.is_contiguous() && xf_mt * 16 >= q.size(0) && out.numel() >= xf_mt * 16 * H * 128)
                                   : out.sizes() == q.sizes()),
              "attn_prefill: out [T, H, 128], or xf_mt >= T / 16 row tiles of fragment-major rows");
  TORCH_CHECK(cu_q.numel() == ctx_lens.numel() + 1 && block_tables.size(0) >= ctx_lens.numel(),
              "cu_q [nseq + 1], ctx_lens [nseq], block_tables [>= nseq, max_blocks]");
  if (rows32) {  // 32 x 32 MFMA kernel, 128 query rows per work item (kernels/attention_prefill32.hip)
    // work [n_workgroups, 4 * NG] of (seq, q_start, t0, t1) (ops.prefill_plan)
    TORCH_CHECK(rows32 == 1, "attn_prefill: rows32 must be 0 or 1");
    TORCH_CHECK(work.dim() == 2 && (work.size(1) == 4 || work.size(1) == 8) && work.is_contiguous(),
                "attn_prefill32 work must be [n, 4 per group] int32");
    check(lsa_attn_prefill32(q.data_ptr(), kc.data_ptr(), vc.data_ptr(), block_tables.data_ptr<int>(),
                             block_tables.size(1), cu_q.data_ptr<int>(), ctx_lens.data_ptr<int>(), work.data_ptr<int>(),
                             work.size(0), H, Hkv, (float)scale, out.data_ptr(), (int)(work.size(1) / 4), (int)xf_mt,
                             cur_stream()),
          "attn_prefill32");
    return;
  }
  check(lsa_attn_prefill(q.data_ptr(), kc.data_ptr(), vc.data_ptr(), block_tables.data_ptr<int>(),
                         block_tables.size(1), cu_q.data_ptr<int>(), ctx_lens.data_ptr<int>(), work.data_ptr<int>(),
                         work.size(0), H, Hkv, (float)scale, out.data_ptr(), (int)xf_mt, cur_stream()),
        "attn_prefill");
}

// decode-state operands of the commit kernels: [B] int32 rows, out_tokens [B, max_new]
void check_state(int64_t B, const at::Tensor& out_tokens, const at::Tensor& gen_len, const at::Tensor& input_ids,
                 const at::Tensor& positions, const at::Tensor& finished, const at::Tensor& eos,
                 const at::Tensor& limit, const at::Tensor& eos_on) {
  for (const at::Tensor* t : {&gen_len, &input_ids, &positions, &finished, &limit, &eos_on}) {
    need(*t, at::kInt, "decode state");
    TORCH_CHECK(t->numel() >= B && t->is_contiguous(), "decode state rows: numel < B");
  }
  need(out_tokens, at::kInt, "out_tokens");
  TORCH_CHECK(out_tokens.dim() == 2 && out_tokens.size(0) >= B && out_tokens.is_contiguous(), "out_tokens [B, max_new]");
  need(eos, at::kInt, "eos");
  TORCH_CHECK(eos.numel() >= 1, "eos: at least one id (-1 = none)");
}

void argmax_commit(const at::Tensor& logits, at::Tensor& part, at::Tensor& out_tokens, at::Tensor& gen_len,
                   at::Tensor& input_ids, at::Tensor& positions, at::Tensor& finished, const at::Tensor& eos,
                   const at::Tensor& limit, const at::Tensor& eos_on) {
  need(logits, at::kFloat, "logits");
  TORCH_CHECK(logits.dim() == 2 && logits.is_contiguous(), "logits: contiguous [B, V]");
  const int B = logits.size(0), V = logits.size(1);
  check_state(B, out_tokens, gen_len, input_ids, positions, finished, eos, limit, eos_on);
  need(part, at::kLong, "part");
  TORCH_CHECK(part.numel() >= (int64_t)B * ((V + 4095) / 4096), "argmax partials too small");
  check(lsa_argmax_commit(logits.data_ptr<float>(), B, V, reinterpret_cast<unsigned long long*>(part.data_ptr()),
                          out_tokens.data_ptr<int>(), out_tokens.size(1), gen_len.data_ptr<int>(),
                          input_ids.data_ptr<int>(), positions.data_ptr<int>(), finished.data_ptr<int>(),
                          eos.data_ptr<int>(), eos.numel(), limit.data_ptr<int>(), eos_on.data_ptr<int>(), cur_stream()),
        "argmax_commit");
}

// speculative decoding: attention of the T = k + 1 verify rows of each of S sequences (kernels/attention_verify.hip):
// q [S, T, H, 128] with block_table [S, max_blocks], pos0 [S] and out [S * T, H * 128]; q [T, H, 128] with one block-table
// row is the one-sequence form
void attn_verify(const at::Tensor& q, const at::Tensor& kc, const at::Tensor& vc, const at::Tensor& block_table,
                 const at::Tensor& pos0, int64_t H, int64_t Hkv, double scale, int64_t chunk_blocks, int64_t nsplit,
                 int64_t unsplit_max, at::Tensor& out, at::Tensor& opart, at::Tensor& mlpart, at::Tensor& counters,
                 const c10::optional<at::Tensor>& ks = c10::nullopt, const c10::optional<at::Tensor>& vs = c10::nullopt) {
  need(q, at::kBFloat16, "q");
  need(out, at::kBFloat16, "out");
  check_cache(kc, vc, ks, vs);  // bf16 cache without scales, e4m3 bytes with both
  need(pos0, at::kInt, "pos0");
  need(block_table, at::kInt, "block_table");
  TORCH_CHECK((q.dim() == 3 || q.dim() == 4) && q.size(-2) == H && q.size(-1) == 128 && q.is_contiguous(),
              "q: contiguous [T, H, 128] or [S, T, H, 128]");
  const int64_t S = q.dim() == 4 ? q.size(0) : 1, T = q.size(-3);
  TORCH_CHECK(H > 0 && Hkv > 0 && H % Hkv == 0 && kc.size(1) == Hkv, "heads: H % Hkv == 0, cache has Hkv heads");
  TORCH_CHECK(T >= 1 && T <= 8 && T * (H / Hkv) <= 16, "attn_verify: T <= 8 and T * H / Hkv <= 16 query rows per kv head");
  TORCH_CHECK(S >= 1 && S <= 8, "attn_verify: 1 <= S <= 8 sequences");
  TORCH_CHECK(S * T <= 32, "attn_verify: S * T <= 32 rows");
  TORCH_CHECK(pos0.numel() >= S && pos0.is_contiguous(), "pos0: one int32 per sequence");
  TORCH_CHECK(block_table.is_contiguous() && block_table.numel() >= 1 &&
                  (q.dim() == 4 ? (block_table.dim() == 2 && block_table.size(0) == S)
                                : (block_table.dim() == 1 || block_table.size(0) == 1)),
              "block_table: one contiguous row [max_blocks], or [S, max_blocks] with q [S, T, H, 128]");
  const int64_t max_blocks = block_table.numel() / S;
  TORCH_CHECK(out.is_contiguous() && out.numel() >= S * T * H * 128, "attn_verify out too small");
  TORCH_CHECK(nsplit >= 1 && nsplit <= 256 && chunk_blocks >= 1, "attn_verify: 1 <= nsplit <= 256, chunk_blocks >= 1");
  need(opart, at::kFloat, "opart");
  need(mlpart, at::kFloat, "mlpart");
  need(counters, at::kInt, "counters");
  TORCH_CHECK(opart.numel() >= S * T * H * nsplit * 128 && mlpart.numel() >= S * T * H * nsplit * 2 &&
                  counters.numel() >= S * Hkv,
              "attn_verify workspace too small");
  TORCH_CHECK(opart.numel() * 4 < 0x7fffffffLL, "opart must stay below 2 GiB (buffer descriptor range)");
  check(lsa_attn_verify(q.data_ptr(), kc.data_ptr(), vc.data_ptr(), block_table.data_ptr<int>(), max_blocks,
                        pos0.data_ptr<int>(), S, T, H, Hkv, (float)scale, chunk_blocks, nsplit, (int)unsplit_max,
                        out.data_ptr(), opart.data_ptr<float>(), mlpart.data_ptr<float>(), counters.data_ptr<int>(),
                        cur_stream(), ptr<const float>(ks), ptr<const float>(vs)),
        "attn_verify");
}

// speculative decoding: the prompt-lookup drafter (kernels/spec.hip); rows = prompt_len.numel()
void spec_draft(const at::Tensor& prompt_tok, const at::Tensor& prompt_len, const at::Tensor& out_tokens,
                const at::Tensor& gen_len, const at::Tensor& input_ids, const at::Tensor& positions, int64_t k,
                int64_t n_max, int64_t n_min, const c10::optional<at::Tensor>& forced, const at::Tensor& spec_ids,
                const at::Tensor& spec_pos, const at::Tensor& spec_draft_out) {
  const int64_t rows = prompt_len.numel();
  for (const at::Tensor* t : {&prompt_tok, &prompt_len, &out_tokens, &gen_len, &input_ids, &positions, &spec_ids,
                              &spec_pos, &spec_draft_out}) {
    need(*t, at::kInt, "spec_draft operand");
    TORCH_CHECK(t->is_contiguous(), "spec_draft operands must be contiguous");
  }
  TORCH_CHECK(rows >= 1 && k >= 1 && k <= 255 && n_max >= 1 && n_min >= 1 && n_min <= n_max,
              "spec_draft: rows >= 1, 1 <= k <= 255, 1 <= n_min <= n_max");
  TORCH_CHECK(prompt_tok.dim() == 2 && prompt_tok.size(0) >= rows && out_tokens.dim() == 2 && out_tokens.size(0) >= rows,
              "spec_draft: prompt_tok [rows, max_len], out_tokens [rows, max_new]");
  TORCH_CHECK(gen_len.numel() >= rows && input_ids.numel() >= rows && positions.numel() >= rows,
              "spec_draft: state rows");
  TORCH_CHECK(spec_ids.numel() >= rows * (k + 1) && spec_pos.numel() >= rows * (k + 1) && spec_draft_out.numel() >= rows * k,
              "spec_draft outputs too small");
  int64_t nf = 0, forced_ld = 0;
  if (forced.has_value()) {
    need(*forced, at::kInt, "forced");
    TORCH_CHECK(forced->is_contiguous() && forced->numel() >= k && forced->numel() % k == 0, "forced: contiguous [nf, k]");
    nf = forced->numel() / k;
    if (forced->dim() == 3) {  // one table per row
      TORCH_CHECK(forced->size(0) >= rows && forced->size(1) >= 1 && forced->size(2) == k,
                  "forced: contiguous [rows, nf, k]");
      nf = forced->size(1);
      forced_ld = nf * k;
    }
  }
  check(lsa_spec_draft(prompt_tok.data_ptr<int>(), prompt_tok.size(1), prompt_len.data_ptr<int>(),
                       out_tokens.data_ptr<int>(), out_tokens.size(1), gen_len.data_ptr<int>(), input_ids.data_ptr<int>(),
                       positions.data_ptr<int>(), rows, k, n_max, n_min, ptr<const int>(forced), nf, forced_ld,
                       spec_ids.data_ptr<int>(), spec_pos.data_ptr<int>(), spec_draft_out.data_ptr<int>(), cur_stream()),
        "spec_draft");
}

// speculative decoding: argmax of the verify rows + in-order commit of each sequence's accepted run into its state row.
// stats [3]: logits [T, V] are the rows of the sequence in state row 0; stats [S, 3]: logits [S * T, V], draft [S, T - 1]
// and state rows 0 .. S - 1
void spec_commit(const at::Tensor& logits, at::Tensor& part, const at::Tensor& draft, at::Tensor& stats,
                 at::Tensor& out_tokens, at::Tensor& gen_len, at::Tensor& input_ids, at::Tensor& positions,
                 at::Tensor& finished, const at::Tensor& eos, const at::Tensor& limit, const at::Tensor& eos_on) {
  need(logits, at::kFloat, "logits");
  TORCH_CHECK(logits.dim() == 2 && logits.is_contiguous() && logits.size(0) >= 2, "logits: contiguous [S * T >= 2, V]");
  need(stats, at::kLong, "stats");
  TORCH_CHECK(stats.is_contiguous() && (stats.dim() == 2 ? stats.size(0) >= 1 && stats.size(1) == 3 : stats.numel() >= 3),
              "spec_commit: stats [3] or [S, 3]");
  const int S = stats.dim() == 2 ? stats.size(0) : 1;
  TORCH_CHECK(logits.size(0) % S == 0 && logits.size(0) / S >= 2 && (S == 1 || logits.size(0) <= 32),
              "spec_commit: logits [S * T, V] with T >= 2 and S * T <= 32");
  const int T = logits.size(0) / S, V = logits.size(1);
  check_state(S, out_tokens, gen_len, input_ids, positions, finished, eos, limit, eos_on);
  need(part, at::kLong, "part");
  TORCH_CHECK(part.numel() >= (int64_t)S * T * ((V + 4095) / 4096), "argmax partials too small");
  need(draft, at::kInt, "draft");
  TORCH_CHECK(draft.numel() >= (int64_t)S * (T - 1) && draft.is_contiguous(), "spec_commit: draft [S, T - 1]");
  check(lsa_spec_commit(logits.data_ptr<float>(), S, T, V, reinterpret_cast<unsigned long long*>(part.data_ptr()),
                        draft.data_ptr<int>(), reinterpret_cast<long long*>(stats.data_ptr<int64_t>()),
                        out_tokens.data_ptr<int>(), out_tokens.size(1), gen_len.data_ptr<int>(),
                        input_ids.data_ptr<int>(), positions.data_ptr<int>(), finished.data_ptr<int>(),
                        eos.data_ptr<int>(), eos.numel(), limit.data_ptr<int>(), eos_on.data_ptr<int>(), cur_stream()),
        "spec_commit");
}

// per-token logprobs (kernels/logprobs.hip).  Workspace of both launches: lp_ms f32 [>= B * ceil(V / 2048) * 2], lp_cand
// int64 [>= B * ceil(V / 2048) * 32]; lp_raw f32 [>= B, V] holds the raw rows between them.
void check_logprob_ws(const char* op, int64_t B, int64_t V, const at::Tensor& lp_k, const at::Tensor& lp_n0,
                      const at::Tensor& gen_len, const at::Tensor& lp_raw, const at::Tensor& lp_ms,
                      const at::Tensor& lp_cand) {
  TORCH_CHECK(B >= 1 && V >= 1 && V <= 262144, op, ": 1 <= V <= 262144 (the sampler's bound), B >= 1");
  for (const at::Tensor* t : {&lp_k, &lp_n0, &gen_len}) {
    need(*t, at::kInt, "logprob state operand");
    TORCH_CHECK(t->is_contiguous() && t->numel() >= B, op, ": lp_k / lp_n0 / gen_len contiguous int32 [>= B]");
  }
  need(lp_raw, at::kFloat, "lp_raw");
  need(lp_ms, at::kFloat, "lp_ms");
  need(lp_cand, at::kLong, "lp_cand");
  TORCH_CHECK(lp_raw.dim() == 2 && lp_raw.size(0) >= B && lp_raw.size(1) == V && lp_raw.is_contiguous(), op,
              ": lp_raw contiguous f32 [>= B, V]");
  const int64_t nch = (V + 2047) / 2048;
  TORCH_CHECK(lp_ms.is_contiguous() && lp_cand.is_contiguous() && lp_ms.numel() >= B * nch * 2 &&
                  lp_cand.numel() >= B * nch * 32,
              op, ": chunk workspaces too small");
}

void logprob_scan(const at::Tensor& logits, const at::Tensor& lp_k, const at::Tensor& finished,
                  const at::Tensor& gen_len, at::Tensor& lp_raw, at::Tensor& lp_ms, at::Tensor& lp_cand,
                  at::Tensor& lp_n0) {
  need(logits, at::kFloat, "logits");
  TORCH_CHECK(logits.dim() == 2 && logits.is_contiguous(), "logprob_scan: logits contiguous [B, V]");
  const int64_t B = logits.size(0), V = logits.size(1);
  check_logprob_ws("logprob_scan", B, V, lp_k, lp_n0, gen_len, lp_raw, lp_ms, lp_cand);
  need(finished, at::kInt, "finished");
  TORCH_CHECK(finished.is_contiguous() && finished.numel() >= B, "logprob_scan: finished contiguous int32 [>= B]");
  check(lsa_logprob_scan(logits.data_ptr<float>(), (int)B, (int)V, lp_k.data_ptr<int>(), finished.data_ptr<int>(),
                         gen_len.data_ptr<int>(), lp_raw.data_ptr<float>(), lp_ms.data_ptr<float>(),
                         reinterpret_cast<unsigned long long*>(lp_cand.data_ptr()), lp_n0.data_ptr<int>(), cur_stream()),
        "logprob_scan");
}

// records: lp_tok f32 of out_tokens' shape, lp_ids int32 / lp_top f32 [rows, max_new, K] with 0 <= K <= 20
void logprob_commit(const at::Tensor& lp_raw, const at::Tensor& lp_ms, const at::Tensor& lp_cand,
                    const at::Tensor& lp_k, at::Tensor& lp_n0, const at::Tensor& gen_len, const at::Tensor& out_tokens,
                    at::Tensor& lp_tok, at::Tensor& lp_ids, at::Tensor& lp_top, int64_t B) {
  need(lp_raw, at::kFloat, "lp_raw");
  TORCH_CHECK(lp_raw.dim() == 2, "logprob_commit: lp_raw [>= B, V]");
  const int64_t V = lp_raw.size(1);
  check_logprob_ws("logprob_commit", B, V, lp_k, lp_n0, gen_len, lp_raw, lp_ms, lp_cand);
  need(out_tokens, at::kInt, "out_tokens");
  need(lp_tok, at::kFloat, "lp_tok");
  need(lp_ids, at::kInt, "lp_ids");
  need(lp_top, at::kFloat, "lp_top");
  TORCH_CHECK(out_tokens.dim() == 2 && out_tokens.size(0) >= B && out_tokens.size(1) >= 1 && out_tokens.is_contiguous(),
              "logprob_commit: out_tokens contiguous [>= B, max_new]");
  TORCH_CHECK(lp_tok.sizes() == out_tokens.sizes() && lp_tok.is_contiguous(),
              "logprob_commit: lp_tok must have out_tokens' shape");
  TORCH_CHECK(lp_ids.dim() == 3 && lp_ids.sizes() == lp_top.sizes() && lp_ids.size(0) == out_tokens.size(0) &&
                  lp_ids.size(1) == out_tokens.size(1) && lp_ids.is_contiguous() && lp_top.is_contiguous(),
              "logprob_commit: lp_ids / lp_top contiguous [rows, max_new, K] over out_tokens' rows");
  TORCH_CHECK(lp_ids.size(2) >= 0 && lp_ids.size(2) <= 20, "logprob_commit: top_logprobs K must be in 0 .. 20");
  check(lsa_logprob_commit(lp_raw.data_ptr<float>(), (int)B, (int)V, lp_ms.data_ptr<float>(),
                           reinterpret_cast<const unsigned long long*>(lp_cand.data_ptr()), lp_k.data_ptr<int>(),
                           lp_n0.data_ptr<int>(), gen_len.data_ptr<int>(), out_tokens.data_ptr<int>(),
                           (int)out_tokens.size(1), lp_tok.data_ptr<float>(), lp_ids.data_ptr<int>(),
                           lp_top.data_ptr<float>(), (int)lp_ids.size(2), cur_stream()),
        "logprob_commit");
}

// the verify-step pair (spec_logprobs): S = lp_k.numel() sequences of T rows; the spec-side workspace sp_raw f32 [32, V],
// sp_ms, sp_cand holds 32 rows whatever S * T is.  S / T / S * T are refused here and in the launcher.
void check_spec_logprob(const char* op, int64_t S, int64_t T, int64_t V, const at::Tensor& lp_k,
                        const at::Tensor& lp_n0, const at::Tensor& gen_len, const at::Tensor& sp_raw,
                        const at::Tensor& sp_ms, const at::Tensor& sp_cand) {
  TORCH_CHECK(T >= 1 && T <= 8 && S >= 1 && S <= 8 && S * T <= 32, op, ": 1 <= T <= 8, 1 <= S <= 8, S * T <= 32");
  TORCH_CHECK(V >= 1 && V <= 262144, op, ": 1 <= V <= 262144 (the sampler's bound)");
  for (const at::Tensor* t : {&lp_k, &lp_n0, &gen_len}) {
    need(*t, at::kInt, "logprob state operand");
    TORCH_CHECK(t->is_contiguous() && t->numel() >= S, op, ": lp_k / lp_n0 / gen_len contiguous int32 [>= S]");
  }
  need(sp_raw, at::kFloat, "spec raw rows");
  need(sp_ms, at::kFloat, "spec lp_ms");
  need(sp_cand, at::kLong, "spec lp_cand");
  TORCH_CHECK(sp_raw.dim() == 2 && sp_raw.size(0) >= 32 && sp_raw.size(1) == V && sp_raw.is_contiguous(), op,
              ": raw rows contiguous f32 [>= 32, V]");
  const int64_t nch = (V + 2047) / 2048;
  TORCH_CHECK(sp_ms.is_contiguous() && sp_cand.is_contiguous() && sp_ms.numel() >= 32 * nch * 2 &&
                  sp_cand.numel() >= 32 * nch * 32,
              op, ": chunk workspaces too small (32 rows)");
}

void spec_logprob_scan(const at::Tensor& logits, int64_t T, const at::Tensor& lp_k, const at::Tensor& finished,
                       const at::Tensor& gen_len, at::Tensor& sp_raw, at::Tensor& sp_ms, at::Tensor& sp_cand,
                       at::Tensor& lp_n0) {
  need(logits, at::kFloat, "logits");
  TORCH_CHECK(logits.dim() == 2 && logits.is_contiguous(), "spec_logprob_scan: logits contiguous [S * T, V]");
  const int64_t S = lp_k.numel(), V = logits.size(1);
  check_spec_logprob("spec_logprob_scan", S, T, V, lp_k, lp_n0, gen_len, sp_raw, sp_ms, sp_cand);
  TORCH_CHECK(logits.size(0) == S * T, "spec_logprob_scan: logits must have S * T rows");
  need(finished, at::kInt, "finished");
  TORCH_CHECK(finished.is_contiguous() && finished.numel() >= S, "spec_logprob_scan: finished contiguous int32 [>= S]");
  check(lsa_spec_logprob_scan(logits.data_ptr<float>(), (int)S, (int)T, (int)V, lp_k.data_ptr<int>(),
                              finished.data_ptr<int>(), gen_len.data_ptr<int>(), sp_raw.data_ptr<float>(),
                              sp_ms.data_ptr<float>(), reinterpret_cast<unsigned long long*>(sp_cand.data_ptr()),
                              lp_n0.data_ptr<int>(), cur_stream()),
        "spec_logprob_scan");
}

// records as logprob_commit's, rows >= S (the per-slot record tensors: sequence s is slot s)
void spec_logprob_commit(int64_t T, const at::Tensor& sp_raw, const at::Tensor& sp_ms, const at::Tensor& sp_cand,
                         const at::Tensor& lp_k, const at::Tensor& lp_n0, const at::Tensor& gen_len,
                         const at::Tensor& out_tokens, at::Tensor& lp_tok, at::Tensor& lp_ids, at::Tensor& lp_top) {
  TORCH_CHECK(sp_raw.dim() == 2, "spec_logprob_commit: raw rows [32, V]");
  const int64_t S = lp_k.numel(), V = sp_raw.size(1);
  check_spec_logprob("spec_logprob_commit", S, T, V, lp_k, lp_n0, gen_len, sp_raw, sp_ms, sp_cand);
  need(out_tokens, at::kInt, "out_tokens");
  need(lp_tok, at::kFloat, "lp_tok");
  need(lp_ids, at::kInt, "lp_ids");
  need(lp_top, at::kFloat, "lp_top");
  TORCH_CHECK(out_tokens.dim() == 2 && out_tokens.size(0) >= S && out_tokens.size(1) >= 1 && out_tokens.is_contiguous(),
              "spec_logprob_commit: out_tokens contiguous [>= S, max_new]");
  TORCH_CHECK(lp_tok.sizes() == out_tokens.sizes() && lp_tok.is_contiguous(),
              "spec_logprob_commit: lp_tok must have out_tokens' shape");
  TORCH_CHECK(lp_ids.dim() == 3 && lp_ids.sizes() == lp_top.sizes() && lp_ids.size(0) == out_tokens.size(0) &&
                  lp_ids.size(1) == out_tokens.size(1) && lp_ids.is_contiguous() && lp_top.is_contiguous(),
              "spec_logprob_commit: lp_ids / lp_top contiguous [rows, max_new, K] over out_tokens' rows");
  TORCH_CHECK(lp_ids.size(2) >= 0 && lp_ids.size(2) <= 20, "spec_logprob_commit: top_logprobs K must be in 0 .. 20");
  check(lsa_spec_logprob_commit(sp_raw.data_ptr<float>(), (int)S, (int)T, (int)V, sp_ms.data_ptr<float>(),
                                reinterpret_cast<const unsigned long long*>(sp_cand.data_ptr()), lp_k.data_ptr<int>(),
                                lp_n0.data_ptr<int>(), gen_len.data_ptr<int>(), out_tokens.data_ptr<int>(),
                                (int)out_tokens.size(1), lp_tok.data_ptr<float>(), lp_ids.data_ptr<int>(),
                                lp_top.data_ptr<float>(), (int)lp_ids.size(2), cur_stream()),
        "spec_logprob_commit");
}

// the prompt pair (prompt-token logprobs): R scored prefill rows of logits [R, V] with their targets (< 0: no record) and
// K per row; ms f32 [>= R * ceil(V / 2048) * 2], cand int64 [>= R * ceil(V / 2048) * 32].  any_k: some row has K > 0
// (the launch form that writes and reads the candidates).
void check_prompt_logprob(const char* op, const at::Tensor& logits, const at::Tensor& targets, const at::Tensor& row_k,
                          const at::Tensor& ms, const at::Tensor& cand) {
  need(logits, at::kFloat, "logits");
  TORCH_CHECK(logits.dim() == 2 && logits.is_contiguous(), op, ": logits contiguous f32 [R, V]");
  const int64_t R = logits.size(0), V = logits.size(1);
  TORCH_CHECK(R >= 1 && V >= 1 && V <= 262144, op, ": 1 <= V <= 262144 (the sampler's bound), R >= 1");
  for (const at::Tensor* t : {&targets, &row_k}) {
    need(*t, at::kInt, "prompt logprob row operand");
    TORCH_CHECK(t->dim() == 1 && t->is_contiguous() && t->numel() == R, op, ": targets / row_k contiguous int32 [R]");
  }
  need(ms, at::kFloat, "ms");
  need(cand, at::kLong, "cand");
  const int64_t nch = (V + 2047) / 2048;
  TORCH_CHECK(ms.is_contiguous() && cand.is_contiguous() && ms.numel() >= R * nch * 2 && cand.numel() >= R * nch * 32,
              op, ": chunk workspaces too small");
}

void prompt_logprob_scan(const at::Tensor& logits, const at::Tensor& targets, const at::Tensor& row_k, bool any_k,
                         at::Tensor& ms, at::Tensor& cand) {
  check_prompt_logprob("prompt_logprob_scan", logits, targets, row_k, ms, cand);
  check(lsa_prompt_logprob_scan(logits.data_ptr<float>(), (int)logits.size(0), (int)logits.size(1),
                                targets.data_ptr<int>(), any_k ? 1 : 0, ms.data_ptr<float>(),
                                reinterpret_cast<unsigned long long*>(cand.data_ptr()), cur_stream()),
        "prompt_logprob_scan");
}

// records: dst_tok f32 [R], dst_ids int32 / dst_top f32 [R, kcap] with 0 <= kcap <= 20
void prompt_logprob_commit(const at::Tensor& logits, const at::Tensor& ms, const at::Tensor& cand,
                           const at::Tensor& targets, const at::Tensor& row_k, bool any_k, at::Tensor& dst_tok,
                           at::Tensor& dst_ids, at::Tensor& dst_top) {
  check_prompt_logprob("prompt_logprob_commit", logits, targets, row_k, ms, cand);
  const int64_t R = logits.size(0);
  need(dst_tok, at::kFloat, "dst_tok");
  need(dst_ids, at::kInt, "dst_ids");
  need(dst_top, at::kFloat, "dst_top");
  TORCH_CHECK(dst_tok.dim() == 1 && dst_tok.numel() == R && dst_tok.is_contiguous(),
              "prompt_logprob_commit: dst_tok contiguous f32 [R]");
  TORCH_CHECK(dst_ids.dim() == 2 && dst_ids.sizes() == dst_top.sizes() && dst_ids.size(0) == R &&
                  dst_ids.is_contiguous() && dst_top.is_contiguous(),
              "prompt_logprob_commit: dst_ids / dst_top contiguous [R, K]");
  TORCH_CHECK(dst_ids.size(1) >= 0 && dst_ids.size(1) <= 20, "prompt_logprob_commit: top_logprobs K must be in 0 .. 20");
  check(lsa_prompt_logprob_commit(logits.data_ptr<float>(), (int)R, (int)logits.size(1), ms.data_ptr<float>(),
                                  reinterpret_cast<const unsigned long long*>(cand.data_ptr()),
                                  targets.data_ptr<int>(), row_k.data_ptr<int>(), any_k ? 1 : 0,
                                  dst_tok.data_ptr<float>(), dst_ids.data_ptr<int>(), dst_top.data_ptr<float>(),
                                  (int)dst_ids.size(1), cur_stream()),
        "prompt_logprob_commit");
}

// regex-constrained decoding: -inf into every logit whose token would kill the row's DFA (kernels/guided.hip).
// Table rows are indexed by rows[b] when given (prefill tail: the sequence's slot), else by b.
void dfa_mask(at::Tensor& logits, const at::Tensor& tok_off, const at::Tensor& tok_blob, const at::Tensor& cls,
              const at::Tensor& trans, const at::Tensor& accept, const at::Tensor& g_dim, const at::Tensor& g_on,
              at::Tensor& g_state, const at::Tensor& g_base, const c10::optional<at::Tensor>& rows,
              const at::Tensor& gen_len, const at::Tensor& input_ids, const at::Tensor& finished,
              const at::Tensor& eos) {
  need(logits, at::kFloat, "logits");
  TORCH_CHECK(logits.dim() == 2 && logits.is_contiguous() && logits.size(0) >= 1 && logits.size(0) <= 65535 &&
                  logits.size(1) >= 1 && logits.numel() < 0x7fffffffLL, "logits: contiguous [1 <= B <= 65535, V]");
  const int64_t B = logits.size(0), V = logits.size(1);
  need(tok_off, at::kInt, "tok_off");
  need(tok_blob, at::kByte, "tok_blob");
  need(cls, at::kByte, "cls");
  need(trans, at::kShort, "trans");
  need(accept, at::kByte, "accept");
  TORCH_CHECK(tok_off.is_contiguous() && tok_off.numel() == V + 1 && tok_blob.is_contiguous() && tok_blob.numel() >= 1,
              "dfa_mask: tok_off [V + 1], tok_blob non-empty");
  TORCH_CHECK(cls.dim() == 2 && cls.size(1) == 256 && cls.is_contiguous(), "cls: contiguous [Bmax, 256]");
  const int64_t Bmax = cls.size(0);
  TORCH_CHECK(trans.dim() == 2 && trans.size(0) == Bmax && trans.size(1) == 32768 && trans.is_contiguous() &&
                  accept.dim() == 2 && accept.size(0) == Bmax && accept.size(1) == 32768 && accept.is_contiguous(),
              "trans / accept: contiguous [Bmax, 32768]");
  TORCH_CHECK(reinterpret_cast<uintptr_t>(trans.data_ptr()) % 16 == 0, "trans must be 16-byte aligned");
  const at::Tensor& g_state_c = g_state;
  for (const at::Tensor* t : {&g_dim, &g_on, &g_state_c, &g_base, &gen_len, &input_ids, &finished, &eos}) {
    need(*t, at::kInt, "dfa_mask state operand");
    TORCH_CHECK(t->is_contiguous(), "dfa_mask state operands must be contiguous");
  }
  TORCH_CHECK(g_dim.numel() == 2 * Bmax && g_state.numel() == 2 * Bmax && g_on.numel() == Bmax && g_base.numel() == Bmax,
              "dfa_mask: g_dim / g_state [Bmax, 2], g_on / g_base [Bmax]");
  TORCH_CHECK(gen_len.numel() >= B && input_ids.numel() >= B && finished.numel() >= B, "dfa_mask: state rows");
  if (rows.has_value()) {
    need(*rows, at::kInt, "rows");
    TORCH_CHECK(rows->is_contiguous() && rows->numel() >= B, "rows: contiguous [B]");
  } else {
    TORCH_CHECK(B <= Bmax, "dfa_mask: more logits rows than table rows");
  }
  check(lsa_dfa_mask(logits.data_ptr<float>(), B, V, tok_off.data_ptr<int>(), tok_blob.data_ptr<uint8_t>(),
                     cls.data_ptr<uint8_t>(), reinterpret_cast<const uint16_t*>(trans.data_ptr<int16_t>()),
                     accept.data_ptr<uint8_t>(), g_dim.data_ptr<int>(), g_on.data_ptr<int>(), g_state.data_ptr<int>(),
                     g_base.data_ptr<int>(), ptr<const int>(rows), gen_len.data_ptr<int>(), input_ids.data_ptr<int>(),
                     finished.data_ptr<int>(), eos.data_ptr<int>(), eos.numel(), cur_stream()),
        "dfa_mask");
}

// Speculative decoding of a constrained request: the mask of the T = k + 1 verify rows of the sequence in state row 0
// (table row r); row t is masked in the DFA state after the input token and drafts 1..t.  g_spec int32 [>= 9]:
// gen_len at the launch, then the T states (kernels/guided.hip dfa_mask_verify_kernel).
// A 2-D g_spec [S, 9] selects the form over S sequences (as the 2-D stats of spec_commit): logits [S * T, V], draft
// [>= S * (T - 1)], sequence s = state row s = table row s (r must be 0), g_spec row s.
void dfa_mask_verify(at::Tensor& logits, const at::Tensor& tok_off, const at::Tensor& tok_blob, const at::Tensor& cls,
                     const at::Tensor& trans, const at::Tensor& accept, const at::Tensor& g_dim, const at::Tensor& g_on,
                     at::Tensor& g_state, const at::Tensor& g_base, int64_t r, const at::Tensor& gen_len,
                     const at::Tensor& input_ids, const at::Tensor& finished, const at::Tensor& eos,
                     const at::Tensor& draft, at::Tensor& g_spec) {
  need(logits, at::kFloat, "logits");
  const bool batch = g_spec.dim() == 2;
  const int64_t S = batch ? g_spec.size(0) : 1;
  TORCH_CHECK(!batch || (S >= 1 && S <= 8 && g_spec.size(1) == 9), "dfa_mask_verify: g_spec [1 <= S <= 8, 1 + 8]");
  TORCH_CHECK(logits.dim() == 2 && logits.is_contiguous() && logits.size(0) % S == 0 && logits.size(0) >= 2 * S &&
                  logits.size(0) <= 8 * S && logits.size(0) <= 32 && logits.size(1) >= 1 &&
                  logits.numel() < 0x7fffffffLL,
              "logits: contiguous [S * T, V >= 1], 2 <= T <= 8 rows per sequence, S * T <= 32");
  const int64_t T = logits.size(0) / S, V = logits.size(1);
  need(tok_off, at::kInt, "tok_off");
  need(tok_blob, at::kByte, "tok_blob");
  need(cls, at::kByte, "cls");
  need(trans, at::kShort, "trans");
  need(accept, at::kByte, "accept");
  TORCH_CHECK(tok_off.is_contiguous() && tok_off.numel() == V + 1 && tok_blob.is_contiguous() && tok_blob.numel() >= 1,
              "dfa_mask_verify: tok_off [V + 1], tok_blob non-empty");
  TORCH_CHECK(cls.dim() == 2 && cls.size(1) == 256 && cls.is_contiguous(), "cls: contiguous [Bmax, 256]");
  const int64_t Bmax = cls.size(0);
  TORCH_CHECK(trans.dim() == 2 && trans.size(0) == Bmax && trans.size(1) == 32768 && trans.is_contiguous() &&
                  accept.dim() == 2 && accept.size(0) == Bmax && accept.size(1) == 32768 && accept.is_contiguous(),
              "trans / accept: contiguous [Bmax, 32768]");
  TORCH_CHECK(reinterpret_cast<uintptr_t>(trans.data_ptr()) % 16 == 0, "trans must be 16-byte aligned");
  const at::Tensor &g_state_c = g_state, &g_spec_c = g_spec;
  for (const at::Tensor* t : {&g_dim, &g_on, &g_state_c, &g_base, &gen_len, &input_ids, &finished, &eos, &draft,
                              &g_spec_c}) {
    need(*t, at::kInt, "dfa_mask_verify state operand");
    TORCH_CHECK(t->is_contiguous(), "dfa_mask_verify state operands must be contiguous");
  }
  TORCH_CHECK(g_dim.numel() == 2 * Bmax && g_state.numel() == 2 * Bmax && g_on.numel() == Bmax && g_base.numel() == Bmax,
              "dfa_mask_verify: g_dim / g_state [Bmax, 2], g_on / g_base [Bmax]");
  TORCH_CHECK(r >= 0 && r < Bmax, "dfa_mask_verify: table row out of range");
  TORCH_CHECK(!batch || (r == 0 && S <= Bmax), "dfa_mask_verify over S sequences: r = 0, S <= Bmax table rows");
  TORCH_CHECK(gen_len.numel() >= S && input_ids.numel() >= S && finished.numel() >= S,
              "dfa_mask_verify: one state row per sequence");
  TORCH_CHECK(draft.numel() >= S * (T - 1) && g_spec.numel() >= 9 * S,
              "dfa_mask_verify: draft [S * (T - 1)], g_spec [S, 1 + 8]");
  if (batch) {
    check(lsa_dfa_mask_verify_batch(logits.data_ptr<float>(), (int)S, (int)T, V, tok_off.data_ptr<int>(),
                                    tok_blob.data_ptr<uint8_t>(), cls.data_ptr<uint8_t>(),
                                    reinterpret_cast<const uint16_t*>(trans.data_ptr<int16_t>()),
                                    accept.data_ptr<uint8_t>(), g_dim.data_ptr<int>(), g_on.data_ptr<int>(),
                                    g_state.data_ptr<int>(), g_base.data_ptr<int>(), 0, gen_len.data_ptr<int>(),
                                    input_ids.data_ptr<int>(), finished.data_ptr<int>(), eos.data_ptr<int>(),
                                    eos.numel(), draft.data_ptr<int>(), g_spec.data_ptr<int>(), cur_stream()),
          "dfa_mask_verify (S sequences)");
    return;
  }
  check(lsa_dfa_mask_verify(logits.data_ptr<float>(), T, V, tok_off.data_ptr<int>(), tok_blob.data_ptr<uint8_t>(),
                            cls.data_ptr<uint8_t>(), reinterpret_cast<const uint16_t*>(trans.data_ptr<int16_t>()),
                            accept.data_ptr<uint8_t>(), g_dim.data_ptr<int>(), g_on.data_ptr<int>(),
                            g_state.data_ptr<int>(), g_base.data_ptr<int>(), (int)r, gen_len.data_ptr<int>(),
                            input_ids.data_ptr<int>(), finished.data_ptr<int>(), eos.data_ptr<int>(), eos.numel(),
                            draft.data_ptr<int>(), g_spec.data_ptr<int>(), cur_stream()),
        "dfa_mask_verify");
}

// After spec_commit: the state after the accepted drafts (g_spec) into the slot the next mask launch advances from.
void dfa_spec_advance(const at::Tensor& g_on, at::Tensor& g_state, const at::Tensor& g_spec, const at::Tensor& gen_len,
                      int64_t r, int64_t k) {
  const at::Tensor& g_state_c = g_state;
  for (const at::Tensor* t : {&g_on, &g_state_c, &g_spec, &gen_len}) {
    need(*t, at::kInt, "dfa_spec_advance operand");
    TORCH_CHECK(t->is_contiguous(), "dfa_spec_advance operands must be contiguous");
  }
  TORCH_CHECK(k >= 1 && k <= 7, "dfa_spec_advance: 1 <= k <= 7");
  TORCH_CHECK(r >= 0 && r < g_on.numel() && g_state.numel() == 2 * g_on.numel(),
              "dfa_spec_advance: g_on [Bmax], g_state [Bmax, 2], 0 <= r < Bmax");
  if (g_spec.dim() == 2) {  // the form over S sequences: sequence s = gen_len[s], g_spec row s, table row s
    const int64_t S = g_spec.size(0);
    TORCH_CHECK(S >= 1 && S <= 8 && g_spec.size(1) == 9 && S * (k + 1) <= 32,
                "dfa_spec_advance: g_spec [1 <= S <= 8, 1 + 8], S * (k + 1) <= 32");
    TORCH_CHECK(r == 0 && S <= g_on.numel() && gen_len.numel() >= S,
                "dfa_spec_advance over S sequences: r = 0, S <= Bmax table rows, gen_len [S]");
    check(lsa_dfa_spec_advance_batch(g_on.data_ptr<int>(), g_state.data_ptr<int>(), g_spec.data_ptr<int>(),
                                     gen_len.data_ptr<int>(), 0, (int)S, (int)k, cur_stream()),
          "dfa_spec_advance (S sequences)");
    return;
  }
  TORCH_CHECK(g_spec.numel() >= 9 && gen_len.numel() >= 1, "dfa_spec_advance: g_spec [1 + 8], gen_len row 0");
  check(lsa_dfa_spec_advance(g_on.data_ptr<int>(), g_state.data_ptr<int>(), g_spec.data_ptr<int>(),
                             gen_len.data_ptr<int>(), (int)r, (int)k, cur_stream()),
        "dfa_spec_advance");
}

// presence / frequency / min_p of the sampled commits: optional f32, one entry per row (sequence); checked before any
// launch
static void sampler_option(const c10::optional<at::Tensor>& t, int rows, const char* name) {
  if (!t.has_value()) return;
  need(*t, at::kFloat, name);
  TORCH_CHECK(t->numel() >= rows && t->is_contiguous(), name, ": one f32 per row");
}

void sample_commit(at::Tensor& logits, at::Tensor& part, at::Tensor& cand, const c10::optional<at::Tensor>& hist,
                   const c10::optional<at::Tensor>& penalty, const c10::optional<at::Tensor>& last_n,
                   const at::Tensor& temperature, const at::Tensor& top_k,
                   const at::Tensor& top_p, const at::Tensor& seeds, at::Tensor& out_tokens, at::Tensor& gen_len,
                   at::Tensor& input_ids, at::Tensor& positions, at::Tensor& finished, const at::Tensor& eos,
                   const at::Tensor& limit, const at::Tensor& eos_on,
                   const c10::optional<at::Tensor>& presence = c10::nullopt,
                   const c10::optional<at::Tensor>& frequency = c10::nullopt,
                   const c10::optional<at::Tensor>& min_p = c10::nullopt) {
  need(logits, at::kFloat, "logits");
  TORCH_CHECK(logits.dim() == 2 && logits.is_contiguous(), "logits: contiguous [B, V]");
  const int B = logits.size(0), V = logits.size(1);
  check_state(B, out_tokens, gen_len, input_ids, positions, finished, eos, limit, eos_on);
  sampler_option(presence, B, "presence");
  sampler_option(frequency, B, "frequency");
  sampler_option(min_p, B, "min_p");
  need(part, at::kLong, "part");
  need(cand, at::kLong, "cand");
  TORCH_CHECK(part.numel() >= (int64_t)B * ((V + 4095) / 4096) && cand.numel() >= (int64_t)B * ((V + 2047) / 2048) * 64,
              "sampling workspace too small");
  need(temperature, at::kFloat, "temperature");
  need(top_p, at::kFloat, "top_p");
  need(top_k, at::kInt, "top_k");
  need(seeds, at::kLong, "seeds");
  TORCH_CHECK(temperature.numel() >= B && top_p.numel() >= B && top_k.numel() >= B && seeds.numel() >= B,
              "sampling parameters: one per row");
  if (hist.has_value()) {
    need(*hist, at::kInt, "hist");
    TORCH_CHECK(hist->dim() == 2 && hist->size(0) >= B && hist->is_contiguous(), "hist [B, W]");
    TORCH_CHECK(penalty.has_value() && penalty->numel() >= B, "repetition penalty: one per row");
  }
  const int window = hist.has_value() ? hist->size(1) : 0;
  check(lsa_sample_commit(logits.data_ptr<float>(), B, V, reinterpret_cast<unsigned long long*>(part.data_ptr()),
                          reinterpret_cast<unsigned long long*>(cand.data_ptr()), ptr<int>(hist), window,
                          ptr<const float>(penalty), ptr<const int>(last_n), temperature.data_ptr<float>(), top_k.data_ptr<int>(),
                          top_p.data_ptr<float>(), reinterpret_cast<const unsigned long long*>(seeds.data_ptr()),
                          out_tokens.data_ptr<int>(), out_tokens.size(1), gen_len.data_ptr<int>(),
                          input_ids.data_ptr<int>(), positions.data_ptr<int>(), finished.data_ptr<int>(),
                          eos.data_ptr<int>(), eos.numel(), limit.data_ptr<int>(), eos_on.data_ptr<int>(),
                          ptr<const float>(presence), ptr<const float>(frequency), ptr<const float>(min_p), cur_stream()),
        "sample_commit");
}

// speculative decoding of sampled requests: penalty + sampled (or, temperature <= 0, argmax) pick of each of the T
// verify rows of a sequence at draw counter gen_len[s] + row, then the in-order commit of the accepted run into state
// row s (ring included).  stats [3]: one sequence, logits [T, V], the parameters are row 0's, picks int32 [T].  stats
// [S, 3]: S sequences as in spec_commit, logits [S * T, V], draft [S, T - 1], hist [>= S, W], every per-sequence
// parameter of >= S entries, the workspace (part, cand, picks) sized for S * T <= 32 rows.
void spec_sample_commit(at::Tensor& logits, const at::Tensor& draft, at::Tensor& stats,
                        const c10::optional<at::Tensor>& hist, const c10::optional<at::Tensor>& penalty,
                        const c10::optional<at::Tensor>& last_n, const at::Tensor& temperature, const at::Tensor& top_k,
                        const at::Tensor& top_p, const at::Tensor& seeds, at::Tensor& out_tokens, at::Tensor& gen_len,
                        at::Tensor& input_ids, at::Tensor& positions, at::Tensor& finished, const at::Tensor& eos,
                        const at::Tensor& limit, const at::Tensor& eos_on, at::Tensor& part, at::Tensor& cand,
                        at::Tensor& picks, const c10::optional<at::Tensor>& presence = c10::nullopt,
                        const c10::optional<at::Tensor>& frequency = c10::nullopt,
                        const c10::optional<at::Tensor>& min_p = c10::nullopt) {
  need(logits, at::kFloat, "logits");
  need(stats, at::kLong, "stats");
  const bool rows = stats.dim() == 2 && stats.size(0) > 1;  // the S-sequence form
  TORCH_CHECK(!rows || stats.size(1) == 3, "spec_sample_commit: stats [3] or [S, 3]");
  const int S = rows ? stats.size(0) : 1;
  TORCH_CHECK(logits.dim() == 2 && logits.is_contiguous() && logits.size(1) >= 1 && logits.numel() < 0x7fffffffLL &&
                  logits.size(0) % S == 0 && logits.size(0) / S >= 2 && logits.size(0) / S <= 8 &&
                  logits.size(0) <= (rows ? 32 : 8),
              "logits: contiguous [S * T, V >= 1] with 2 <= T <= 8 and S * T <= 32");
  const int T = logits.size(0) / S, V = logits.size(1);
  check_state(S, out_tokens, gen_len, input_ids, positions, finished, eos, limit, eos_on);
  need(part, at::kLong, "part");
  need(cand, at::kLong, "cand");
  need(picks, at::kInt, "picks");
  TORCH_CHECK(part.numel() >= (int64_t)S * T * ((V + 4095) / 4096) &&
                  cand.numel() >= (int64_t)S * T * ((V + 2047) / 2048) * 64 && picks.numel() >= S * T &&
                  part.is_contiguous() && cand.is_contiguous() && picks.is_contiguous(),
              "spec_sample_commit workspace too small");
  need(draft, at::kInt, "draft");
  TORCH_CHECK(draft.numel() >= (int64_t)S * (T - 1) && draft.is_contiguous() && stats.numel() >= 3 * S &&
                  stats.is_contiguous(),
              "spec_sample_commit: draft [S, T - 1], stats [3] or [S, 3]");
  need(temperature, at::kFloat, "temperature");
  need(top_p, at::kFloat, "top_p");
  need(top_k, at::kInt, "top_k");
  need(seeds, at::kLong, "seeds");
  TORCH_CHECK(temperature.numel() >= S && top_p.numel() >= S && top_k.numel() >= S && seeds.numel() >= S,
              "sampling parameters: one per sequence");
  if (hist.has_value()) {
    need(*hist, at::kInt, "hist");
    TORCH_CHECK(hist->dim() == 2 && hist->size(0) >= S && hist->size(1) >= 1 && hist->is_contiguous(), "hist [S, W]");
    TORCH_CHECK(penalty.has_value() && penalty->numel() >= S, "repetition penalty: one per sequence");
    need(*penalty, at::kFloat, "penalty");
  }
  if (last_n.has_value()) {
    need(*last_n, at::kInt, "last_n");
    TORCH_CHECK(last_n->numel() >= S, "last_n: one per sequence");
  }
  sampler_option(presence, S, "presence");
  sampler_option(frequency, S, "frequency");
  sampler_option(min_p, S, "min_p");
  const int window = hist.has_value() ? hist->size(1) : 0;
  check(lsa_spec_sample_commit(logits.data_ptr<float>(), S, T, V, draft.data_ptr<int>(),
                               reinterpret_cast<long long*>(stats.data_ptr<int64_t>()), ptr<int>(hist), window,
                               ptr<const float>(penalty), ptr<const int>(last_n), temperature.data_ptr<float>(),
                               top_k.data_ptr<int>(), top_p.data_ptr<float>(),
                               reinterpret_cast<const unsigned long long*>(seeds.data_ptr()), out_tokens.data_ptr<int>(),
                               out_tokens.size(1), gen_len.data_ptr<int>(), input_ids.data_ptr<int>(),
                               positions.data_ptr<int>(), finished.data_ptr<int>(), eos.data_ptr<int>(), eos.numel(),
                               limit.data_ptr<int>(), eos_on.data_ptr<int>(),
                               reinterpret_cast<unsigned long long*>(part.data_ptr()),
                               reinterpret_cast<unsigned long long*>(cand.data_ptr()), picks.data_ptr<int>(),
                               ptr<const float>(presence), ptr<const float>(frequency), ptr<const float>(min_p),
                               cur_stream()),
        "spec_sample_commit");
}

// per-token fp8 quantisation of bf16 rows: x8 [M, K] uint8 (e4m3fn bits), sx [M] f32 (amax / 448)
void quant_rows_fp8(const at::Tensor& x, at::Tensor& x8, at::Tensor& sx) {
  need(x, at::kBFloat16, "x");
  need(sx, at::kFloat, "sx");
  TORCH_CHECK(x.dim() == 2 && x.stride(1) == 1, "x must be a row-major matrix");
  const int M = x.size(0), K = x.size(1);
  TORCH_CHECK(on_dev(x8) && x8.element_size() == 1 && x8.dim() == 2 && x8.size(0) >= M && x8.size(1) >= K &&
                  x8.stride(1) == 1, "x8 must be a row-major [M, K] 1-byte tensor");
  TORCH_CHECK(sx.numel() >= M, "sx too small");
  check(lsa_quant_rows_fp8(x.data_ptr(), x.stride(0), M, K, x8.data_ptr(), x8.stride(0), sx.data_ptr<float>(),
                           cur_stream()),
        "quant_rows_fp8");
}

// W8A8 large-M linear layer on the block-scaled fp8 MFMA (kernels/gemm_fp8_tile.hip)
void fp8_gemm_t256(const at::Tensor& x8, const at::Tensor& sx, const at::Tensor& wq, const at::Tensor& sw, int64_t N,
                   at::Tensor& out, int64_t epi, int64_t splitk) {
  need(sx, at::kFloat, "sx");
  need(sw, at::kFloat, "sw");
  TORCH_CHECK(on_dev(x8) && x8.element_size() == 1 && x8.dim() == 2 && x8.stride(1) == 1, "x8: [M, K] bytes");
  const int M = x8.size(0), K = x8.size(1);
  TORCH_CHECK(on_dev(wq) && wq.element_size() == 1 && wq.numel() == N * K, "wq must be N*K fp8 bytes");
  TORCH_CHECK(sx.numel() >= M && sw.numel() >= N, "scale sizes");
  if (epi == 1) {
    need(out, at::kFloat, "out");
    TORCH_CHECK(out.numel() >= splitk * M * N, "f32 out too small");
  } else {
    need(out, at::kBFloat16, "out");
    TORCH_CHECK(out.numel() >= M * (epi == 2 ? N / 2 : N), "bf16 out too small");
  }
  check(lsa_fp8_gemm_t256(x8.data_ptr(), x8.stride(0), sx.data_ptr<float>(), M, K, wq.data_ptr(), sw.data_ptr<float>(),
                          N, out.data_ptr(), epi, splitk, cur_stream()),
        "fp8_gemm_t256");
}

void fp8_dequant(const at::Tensor& wq, const at::Tensor& wscale, int64_t N, int64_t K, at::Tensor& wf) {
  need(wscale, at::kFloat, "wscale");
  need(wf, at::kBFloat16, "wf");
  TORCH_CHECK(wq.numel() == N * K && wf.numel() >= N * K, "fp8_dequant size mismatch");
  check(lsa_fp8_dequant(wq.data_ptr(), wscale.data_ptr<float>(), N, K, wf.data_ptr(), cur_stream()), "fp8_dequant");
}

// ---- one-shot IPC all-reduce (kernels/allreduce.hip); regions are raw device addresses (int64)
int64_t ar_alloc(int64_t bytes) {
  void* p = nullptr;
  check(lsa_ar_alloc((size_t)bytes, &p), "ar_alloc");
  return reinterpret_cast<int64_t>(p);
}

#ifndef LSA_BINDINGS_SELFTEST
py::bytes ar_handle(int64_t p) {
  char h[64];
  check(lsa_ar_handle(reinterpret_cast<void*>(p), h), "ar_handle");
  return py::bytes(h, 64);
}
#endif

int64_t ar_open(const std::string& h) {
  TORCH_CHECK(h.size() == 64, "IPC handle must be 64 bytes");
  void* p = nullptr;
  check(lsa_ar_open(h.data(), &p), "ar_open");
  return reinterpret_cast<int64_t>(p);
}

void ar_run(at::Tensor& data, const c10::optional<at::Tensor>& out, const at::Tensor& regions, int64_t rank,
            int64_t maxb, int64_t nblocks, int64_t timeout_ticks, at::Tensor& err, int64_t nslab = 1,
            const c10::optional<at::Tensor>& res_h = c10::nullopt, const c10::optional<at::Tensor>& res_xn = c10::nullopt,
            const c10::optional<at::Tensor>& res_ss = c10::nullopt, int64_t res_xmt = 0, int64_t mode = 0) {
  // nslab > 1: data is [nslab, n] split-K slabs; the sum lands in slab 0.  mode: bit 0 bf16 payload, bit 1 two-shot
  // (sums only; the caller sized the regions for the two-shot result area)
  need(data, at::kFloat, "data");
  need(regions, at::kLong, "regions");
  need(err, at::kInt, "err");
  TORCH_CHECK(regions.numel() >= 2 && regions.numel() <= 8 && rank >= 0 && rank < regions.numel(),
              "all-reduce: 2..8 regions and 0 <= rank < world");
  TORCH_CHECK(nslab >= 1 && data.numel() % nslab == 0, "all-reduce: numel must split into nslab slabs");
  const int64_t n = data.numel() / nslab;
  TORCH_CHECK(data.is_contiguous() && n % 4 == 0, "all-reduce data: contiguous, slab numel % 4 == 0");
  TORCH_CHECK(reinterpret_cast<uintptr_t>(data.data_ptr()) % 16 == 0, "all-reduce data must be 16-B aligned");
  TORCH_CHECK(n * 4 <= maxb, "all-reduce payload exceeds the registered slot size");
  if (out.has_value()) {
    TORCH_CHECK(nslab == 1, "all-gather takes one slab");
    need(*out, at::kFloat, "out");
    TORCH_CHECK(out->is_contiguous() && out->numel() == n * regions.numel(), "all-gather out size");
  }
  TORCH_CHECK(mode >= 0 && mode <= 3 && (mode == 0 || !out.has_value()), "all-reduce mode: 0..3, sums only");
  int64_t D = 0;
  if (res_h.has_value()) {  // residual epilogue: h [rows, D] f32 += the sum; xn = bf16(h); ss[rows] += sum h^2 (Q24)
    TORCH_CHECK(!out.has_value() && res_xn.has_value() && res_ss.has_value(), "all-reduce residual: h, xn, ss");
    need(*res_h, at::kFloat, "res_h");
    need(*res_xn, at::kBFloat16, "res_xn");
    need(*res_ss, at::kLong, "res_ss");
    TORCH_CHECK(res_h->dim() == 2 && res_h->is_contiguous() && res_h->numel() == n, "all-reduce residual: h [rows, D]");
    D = res_h->size(1);
    const int64_t rows = res_h->size(0);
    TORCH_CHECK(D % 256 == 0, "all-reduce residual: D % 256 == 0");
    TORCH_CHECK(res_ss->numel() >= rows && res_xn->is_contiguous() &&
                    res_xn->numel() >= (res_xmt ? res_xmt * 16 : rows) * D && (!res_xmt || rows <= 16 * res_xmt),
                "all-reduce residual: ss / xn too small");
  }
  check(lsa_ar_run(data.data_ptr<float>(), n, ptr<float>(out), reinterpret_cast<uint8_t* const*>(regions.data_ptr()),
                   rank, regions.numel(), maxb, nblocks, timeout_ticks, err.data_ptr<int>(), nslab, n,
                   res_h.has_value() ? res_h->data_ptr<float>() : nullptr, res_xn.has_value() ? res_xn->data_ptr() : nullptr,
                   res_ss.has_value() ? reinterpret_cast<long long*>(res_ss->data_ptr<int64_t>()) : nullptr, (int)D,
                   (int)res_xmt, (int)mode, cur_stream()),
        "ar_run");
}

// ---------------------------------------------------------------------------------------- latency path (B <= 4)
}  // namespace

#ifndef LSA_BINDINGS_SELFTEST
PYBIND11_MODULE(TORCH_EXTENSION_NAME, m) {
  m.doc() = "gfx950 HIP kernels for the MI355X NL->SQL / Spark-error inference engine";
  m.def("gemm", &gemm, py::arg("x"), py::arg("wf"), py::arg("N"), py::arg("out"), py::arg("epi"), py::arg("nb"),
        py::arg("splitk"), py::arg("waves") = 4, py::arg("div") = 4, py::arg("xlds") = 0,
        py::arg("rowss") = py::none(), py::arg("eps") = 1e-5, py::arg("h") = py::none(), py::arg("xout") = py::none(), py::arg("xmt") = 0, py::arg("ss_out") = py::none(), py::arg("tickets") = py::none());
  m.def("gemm_xf", &gemm_xf, py::arg("xf"), py::arg("M"), py::arg("K"), py::arg("wf"), py::arg("N"), py::arg("out"),
        py::arg("epi"), py::arg("nb"), py::arg("splitk"), py::arg("waves") = 4, py::arg("div") = 4,
        py::arg("rowss") = py::none(), py::arg("eps") = 1e-5, py::arg("h") = py::none(), py::arg("xout") = py::none(), py::arg("xmt") = 0, py::arg("ss_out") = py::none(), py::arg("tickets") = py::none());
  m.def("z12_gemm_xf", &z12_gemm_xf, py::arg("xf"), py::arg("M"), py::arg("K"), py::arg("lo"), py::arg("hi"),
        py::arg("esc"), py::arg("base"), py::arg("N"), py::arg("out"), py::arg("epi"), py::arg("nb"), py::arg("splitk"),
        py::arg("waves") = 4, py::arg("div") = 4, py::arg("rowss") = py::none(), py::arg("eps") = 1e-5);
  m.def("gemm_sk", &gemm_sk, py::arg("x"), py::arg("wf"), py::arg("N"), py::arg("out"), py::arg("epi"), py::arg("ws"),
        py::arg("tickets"), py::arg("ncu"), py::arg("min_share") = 0, py::arg("cfg") = -1, py::arg("xf") = 0,
        py::arg("rows") = 0);
  m.def("gemm_sk_rope", &gemm_sk_rope, py::arg("x"), py::arg("wf"), py::arg("ws"), py::arg("tickets"), py::arg("ncu"),
        py::arg("min_share"), py::arg("cfg"), py::arg("pos"), py::arg("tok_seq"), py::arg("block_tables"),
        py::arg("cos_t"), py::arg("sin_t"), py::arg("q_out"), py::arg("kc"), py::arg("vc"), py::arg("H"), py::arg("Hkv"),
        py::arg("xf") = 0, py::arg("rows") = 0);
  m.def("gemm_sk_epilogue", [](int64_t mode) { lsa_gemm_sk_epilogue((int)mode); });
  m.def("gemm_sk_nbuf", [](int64_t n) { lsa_gemm_sk_nbuf((int)n); });
  m.def("gemm_sk_one_phase", [](int64_t on) { lsa_gemm_sk_one_phase((int)on); });
  m.def("rmsnorm_xf_tile_min", [](int64_t rows) { lsa_rmsnorm_xf_tile_min((int)rows); });
  m.def("gemm_sk_ws_bytes", [](int64_t ncu) { return lsa_gemm_sk_ws_bytes((int)ncu); });
  m.def("gemm_sk_tickets", [](int64_t ncu) { return (int64_t)lsa_gemm_sk_tickets((int)ncu); });
  m.def("fp4_gemm", &fp4_gemm, py::arg("x"), py::arg("wq"), py::arg("sw"), py::arg("N"), py::arg("out"), py::arg("epi"),
        py::arg("nb"), py::arg("splitk"), py::arg("waves") = 4, py::arg("rowss") = py::none(), py::arg("eps") = 1e-5,
        py::arg("h") = py::none(), py::arg("xout") = py::none(), py::arg("xmt") = 0, py::arg("ss_out") = py::none(),
        py::arg("tickets") = py::none());
  m.def("fp4_gemm_xf", &fp4_gemm_xf, py::arg("xf"), py::arg("M"), py::arg("K"), py::arg("wq"), py::arg("sw"),
        py::arg("N"), py::arg("out"), py::arg("epi"), py::arg("nb"), py::arg("splitk"), py::arg("waves") = 4,
        py::arg("rowss") = py::none(), py::arg("eps") = 1e-5, py::arg("h") = py::none(), py::arg("xout") = py::none(),
        py::arg("xmt") = 0, py::arg("ss_out") = py::none(), py::arg("tickets") = py::none());
  m.def("fp4_dequant", &fp4_dequant);
  m.def("q4_gemm", &q4_gemm, py::arg("x"), py::arg("wq"), py::arg("dw"), py::arg("N"), py::arg("out"), py::arg("epi"),
        py::arg("nb"), py::arg("splitk"), py::arg("waves") = 4, py::arg("rowss") = py::none(), py::arg("eps") = 1e-5);
  m.def("q4_gemm_xf", &q4_gemm_xf, py::arg("xf"), py::arg("M"), py::arg("K"), py::arg("wq"), py::arg("dw"),
        py::arg("N"), py::arg("out"), py::arg("epi"), py::arg("nb"), py::arg("splitk"), py::arg("waves") = 4,
        py::arg("rowss") = py::none(), py::arg("eps") = 1e-5);
  m.def("q4_dequant", &q4_dequant);
  m.def("fp8_gemm", &fp8_gemm, py::arg("x"), py::arg("wq"), py::arg("wscale"), py::arg("N"), py::arg("out"),
        py::arg("epi"), py::arg("nb"), py::arg("splitk"), py::arg("waves") = 4, py::arg("depth") = 1,
        py::arg("rowss") = py::none(), py::arg("eps") = 1e-5, py::arg("h") = py::none(), py::arg("xout") = py::none(), py::arg("xmt") = 0, py::arg("ss_out") = py::none(), py::arg("tickets") = py::none());
  m.def("fp8_gemm_xf", &fp8_gemm_xf, py::arg("xf"), py::arg("M"), py::arg("K"), py::arg("wq"), py::arg("wscale"),
        py::arg("N"), py::arg("out"), py::arg("epi"), py::arg("nb"), py::arg("splitk"), py::arg("waves") = 4,
        py::arg("depth") = 1,
        py::arg("rowss") = py::none(), py::arg("eps") = 1e-5, py::arg("h") = py::none(), py::arg("xout") = py::none(), py::arg("xmt") = 0, py::arg("ss_out") = py::none(), py::arg("tickets") = py::none());
  m.def("prefetch", &prefetch, py::arg("tensors"), py::arg("bytes"), py::arg("wgs") = 512);
  m.def("res_add_ss", &res_add_ss, py::arg("h"), py::arg("parts"), py::arg("nparts"), py::arg("part_stride"),
        py::arg("xn"), py::arg("rows"), py::arg("D"), py::arg("xf_mt"), py::arg("ss_out"));
  m.def("add_rmsnorm", &add_rmsnorm, py::arg("h"), py::arg("parts"), py::arg("nparts"), py::arg("part_stride"),
        py::arg("ids"), py::arg("emb"), py::arg("row_idx"), py::arg("write_h"), py::arg("w"), py::arg("eps"),
        py::arg("xn"), py::arg("rows"), py::arg("xf_mt") = 0, py::arg("ss_out") = py::none(), py::arg("ss_ld") = 0,
        py::arg("ss_nzero") = 0, py::arg("x8") = py::none(), py::arg("sx8") = py::none());
  m.def("a8_gemm", &a8_gemm, py::arg("x8"), py::arg("s8"), py::arg("sx"), py::arg("M"), py::arg("K"), py::arg("wq"),
        py::arg("wscale"), py::arg("wsc8"), py::arg("N"), py::arg("out"), py::arg("out_s8"), py::arg("epi"), py::arg("nb"),
        py::arg("splitk"), py::arg("waves"), py::arg("depth"), py::arg("xfo"), py::arg("rowss") = py::none(),
        py::arg("eps") = 1e-5);
  m.def("quant_xf8_blocks", &quant_xf8_blocks, py::arg("x"), py::arg("mt"), py::arg("blk"), py::arg("x8"), py::arg("s8"));
  m.def("quant_xf8", &quant_xf8, py::arg("x"), py::arg("mt"), py::arg("x8"), py::arg("sx"));
  m.def("attn_set_stamps", &attn_set_stamps, py::arg("stamps") = py::none());
  m.def("sk_set_stamps", &sk_set_stamps, py::arg("stamps") = py::none());
  m.def("attn_prefill_set_stamps", &attn_prefill_set_stamps, py::arg("stamps") = py::none());
  m.def("rope_append", &rope_append, py::arg("qkv"), py::arg("pos"), py::arg("tok_seq"), py::arg("block_tables"),
        py::arg("cos"), py::arg("sin"), py::arg("q_out"), py::arg("kc"), py::arg("vc"), py::arg("H"), py::arg("Hkv"),
        py::arg("ks") = py::none(), py::arg("vs") = py::none());
  m.def("kv8_dequant", &kv8_dequant);
  m.def("kv_copy_blocks", &kv_copy_blocks, py::arg("kv"), py::arg("kv_scale"), py::arg("pairs"));
  m.def("kv_shift", &kv_shift, py::arg("kv"), py::arg("moves"), py::arg("cos"), py::arg("sin"));
  m.def("kv_shift8", &kv_shift8, py::arg("kv"), py::arg("kv_scale"), py::arg("moves"), py::arg("cos"), py::arg("sin"));
  m.def("embed_rowscale", &embed_rowscale, py::arg("h"), py::arg("parts"), py::arg("tseq"), py::arg("cu"),
        py::arg("meta"), py::arg("eps"), py::arg("rs"));
  m.def("embed_pool", &embed_pool, py::arg("h"), py::arg("parts"), py::arg("cu"), py::arg("meta"), py::arg("rs"),
        py::arg("gamma"), py::arg("acc"));
  m.def("embed_finish", &embed_finish, py::arg("meta"), py::arg("acc"), py::arg("out"));
  m.def("silu_mul", &silu_mul);
  m.def("attn_decode", &attn_decode, py::arg("q"), py::arg("kc"), py::arg("vc"), py::arg("block_tables"),
        py::arg("pos"), py::arg("H"), py::arg("Hkv"), py::arg("scale"), py::arg("chunk_blocks"), py::arg("nsplit"),
        py::arg("out"), py::arg("opart"), py::arg("mlpart"), py::arg("counters"), py::arg("xf_mt") = 0,
        py::arg("qkv_parts") = py::none(),
        py::arg("cos") = py::none(), py::arg("sin") = py::none(), py::arg("unsplit_max") = 4,
        py::arg("ks") = py::none(), py::arg("vs") = py::none(), py::arg("out_s8") = py::none(),
        py::arg("rowss") = py::none(), py::arg("eps") = 1e-5, py::arg("hidden") = 0);
  m.def("a8_gemm_rr", &a8_gemm_rr, py::arg("h"), py::arg("parts"), py::arg("h_out"), py::arg("wq"), py::arg("wscale"),
        py::arg("wsc8"), py::arg("N"), py::arg("out"), py::arg("out_s8"), py::arg("epi"), py::arg("nb"), py::arg("splitk"),
        py::arg("waves"), py::arg("depth"), py::arg("ss_out") = py::none(), py::arg("eps") = 1e-5);
  m.def("gemm_rr", &gemm_rr, py::arg("h"), py::arg("parts"), py::arg("h_out"), py::arg("wf"), py::arg("N"),
        py::arg("out"), py::arg("epi"), py::arg("nb"), py::arg("splitk"), py::arg("waves"), py::arg("div"),
        py::arg("ss_out") = py::none(), py::arg("eps") = 1e-5);
  m.def("attn_prefill", &attn_prefill, py::arg("q"), py::arg("kc"), py::arg("vc"), py::arg("block_tables"),
        py::arg("cu_q"), py::arg("ctx_lens"), py::arg("work"), py::arg("H"), py::arg("Hkv"), py::arg("scale"),
        py::arg("out"), py::arg("rows32") = 0, py::arg("xf_mt") = 0);
  m.def("argmax_commit", &argmax_commit);
  m.def("sample_commit", &sample_commit, py::arg("logits"), py::arg("part"), py::arg("cand"), py::arg("hist"),
        py::arg("penalty"), py::arg("last_n"), py::arg("temperature"), py::arg("top_k"), py::arg("top_p"),
        py::arg("seeds"), py::arg("out_tokens"), py::arg("gen_len"), py::arg("input_ids"), py::arg("positions"),
        py::arg("finished"), py::arg("eos"), py::arg("limit"), py::arg("eos_on"), py::arg("presence") = py::none(),
        py::arg("frequency") = py::none(), py::arg("min_p") = py::none());
  m.def("attn_verify", &attn_verify, py::arg("q"), py::arg("kc"), py::arg("vc"), py::arg("block_table"),
        py::arg("pos0"), py::arg("H"), py::arg("Hkv"), py::arg("scale"), py::arg("chunk_blocks"), py::arg("nsplit"),
        py::arg("unsplit_max"), py::arg("out"), py::arg("opart"), py::arg("mlpart"), py::arg("counters"),
        py::arg("ks") = py::none(), py::arg("vs") = py::none());
  m.def("spec_draft", &spec_draft, py::arg("prompt_tok"), py::arg("prompt_len"), py::arg("out_tokens"),
        py::arg("gen_len"), py::arg("input_ids"), py::arg("positions"), py::arg("k"), py::arg("n_max"), py::arg("n_min"),
        py::arg("forced"), py::arg("spec_ids"), py::arg("spec_pos"), py::arg("spec_draft"));
  m.def("spec_commit", &spec_commit);
  m.def("spec_sample_commit", &spec_sample_commit, py::arg("logits"), py::arg("draft"), py::arg("stats"),
        py::arg("hist"), py::arg("penalty"), py::arg("last_n"), py::arg("temperature"), py::arg("top_k"),
        py::arg("top_p"), py::arg("seeds"), py::arg("out_tokens"), py::arg("gen_len"), py::arg("input_ids"),
        py::arg("positions"), py::arg("finished"), py::arg("eos"), py::arg("limit"), py::arg("eos_on"), py::arg("part"),
        py::arg("cand"), py::arg("picks"), py::arg("presence") = py::none(), py::arg("frequency") = py::none(),
        py::arg("min_p") = py::none());
  m.def("logprob_scan", &logprob_scan, py::arg("logits"), py::arg("lp_k"), py::arg("finished"), py::arg("gen_len"),
        py::arg("lp_raw"), py::arg("lp_ms"), py::arg("lp_cand"), py::arg("lp_n0"));
  m.def("logprob_commit", &logprob_commit, py::arg("lp_raw"), py::arg("lp_ms"), py::arg("lp_cand"), py::arg("lp_k"),
        py::arg("lp_n0"), py::arg("gen_len"), py::arg("out_tokens"), py::arg("lp_tok"), py::arg("lp_ids"),
        py::arg("lp_top"), py::arg("B"));
  m.def("spec_logprob_scan", &spec_logprob_scan, py::arg("logits"), py::arg("T"), py::arg("lp_k"), py::arg("finished"),
        py::arg("gen_len"), py::arg("sp_raw"), py::arg("sp_ms"), py::arg("sp_cand"), py::arg("lp_n0"));
  m.def("spec_logprob_commit", &spec_logprob_commit, py::arg("T"), py::arg("sp_raw"), py::arg("sp_ms"),
        py::arg("sp_cand"), py::arg("lp_k"), py::arg("lp_n0"), py::arg("gen_len"), py::arg("out_tokens"),
        py::arg("lp_tok"), py::arg("lp_ids"), py::arg("lp_top"));
  m.def("prompt_logprob_scan", &prompt_logprob_scan, py::arg("logits"), py::arg("targets"), py::arg("row_k"),
        py::arg("any_k"), py::arg("ms"), py::arg("cand"));
  m.def("prompt_logprob_commit", &prompt_logprob_commit, py::arg("logits"), py::arg("ms"), py::arg("cand"),
        py::arg("targets"), py::arg("row_k"), py::arg("any_k"), py::arg("dst_tok"), py::arg("dst_ids"),
        py::arg("dst_top"));
  m.def("dfa_mask", &dfa_mask, py::arg("logits"), py::arg("tok_off"), py::arg("tok_blob"), py::arg("cls"),
        py::arg("trans"), py::arg("accept"), py::arg("g_dim"), py::arg("g_on"), py::arg("g_state"), py::arg("g_base"),
        py::arg("rows"), py::arg("gen_len"), py::arg("input_ids"), py::arg("finished"), py::arg("eos"));
  m.def("dfa_mask_verify", &dfa_mask_verify, py::arg("logits"), py::arg("tok_off"), py::arg("tok_blob"), py::arg("cls"),
        py::arg("trans"), py::arg("accept"), py::arg("g_dim"), py::arg("g_on"), py::arg("g_state"), py::arg("g_base"),
        py::arg("r"), py::arg("gen_len"), py::arg("input_ids"), py::arg("finished"), py::arg("eos"), py::arg("draft"),
        py::arg("g_spec"));
  m.def("dfa_spec_advance", &dfa_spec_advance, py::arg("g_on"), py::arg("g_state"), py::arg("g_spec"),
        py::arg("gen_len"), py::arg("r"), py::arg("k"));
  m.def("fp8_dequant", &fp8_dequant);
  m.def("quant_rows_fp8", &quant_rows_fp8);
  m.def("fp8_gemm_t256", &fp8_gemm_t256, py::arg("x8"), py::arg("sx"), py::arg("wq"), py::arg("sw"), py::arg("N"),
        py::arg("out"), py::arg("epi"), py::arg("splitk") = 1);
  m.def("silu_parts", [](const at::Tensor& parts, at::Tensor& out) {
    // parts: f32 [S, M, 2F] (gate/up interleaved per 16 rows) -> out bf16 [M, F] = silu(gate) * up
    need(parts, at::kFloat, "parts");
    need(out, at::kBFloat16, "out");
    const int S = parts.size(0), M = parts.size(1), F = parts.size(2) / 2;
    check(lsa_silu_parts(parts.data_ptr<float>(), S, parts.stride(0), M, F, out.data_ptr(), cur_stream()),
          "silu_parts");
  });
  m.def("silu_bf16", &silu_bf16);
  m.def("ar_alloc", &ar_alloc);
  m.def("ar_free", [](int64_t p) { check(lsa_ar_free(reinterpret_cast<void*>(p)), "ar_free"); });
  m.def("ar_handle", &ar_handle);
  m.def("ar_open", &ar_open);
  m.def("ar_close", [](int64_t p) { check(lsa_ar_close(reinterpret_cast<void*>(p)), "ar_close"); });
  m.def("ar_run", &ar_run, py::arg("data"), py::arg("out"), py::arg("regions"), py::arg("rank"), py::arg("maxb"),
        py::arg("nblocks"), py::arg("timeout_ticks"), py::arg("err"), py::arg("nslab") = 1,
        py::arg("res_h") = py::none(), py::arg("res_xn") = py::none(), py::arg("res_ss") = py::none(),
        py::arg("res_xmt") = 0, py::arg("mode") = 0);
  m.def("ar_wallclock_khz", []() {
    int k = 0;
    check(lsa_ar_wallclock_khz(&k), "ar_wallclock_khz");
    return k;
  });
  m.attr("ar_max_world") = lsa_ar_max_world();
  m.attr("ar_header_bytes") = lsa_ar_header_bytes();
  m.attr("prefill_qblock") = lsa_prefill_qblock();
  m.attr("arch") = "gfx950";
}
#endif  // LSA_BINDINGS_SELFTEST
