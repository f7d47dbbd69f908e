// fc weight-gradient fused with the SGD step as a STREAM over the parameters (gfx950).
//
// Same arithmetic as gemm_glds.hip's EPI_F32_SGD epilogue -- C[j][i] = alpha * sum_k x[k][i] dy[k][j]
// by v_mfma_f32_16x16x32_bf16 (x as A, dy as B, K in ascending 32-steps from a zero accumulator,
// whole 64-k tiles with zeros past K), then sgd_step on (w, m) and the bf16 shadow -- so the
// result is bitwise that kernel's.  What differs is the shape of the work, which follows the
// 18 bytes per parameter of the update instead of the (tiny, K = batch) GEMM:
//   * a block walks a run of 128-column chunks (nin) of a strip of 64 output rows (nout); the
//     strip's dy fragments are read once per run, through LDS into registers, and stay there for
//     every chunk;
//   * a wave's part of a chunk is 16 rows x 128 columns: every w / m / wb wave instruction covers
//     two whole 512-byte row runs;
//   * the w / m loads run a chunk ahead of their use in a rolling register window: the loads of
//     slot s of the next chunk are issued BEFORE the stores of slot s of this one (vmcnt retires in
//     issue order, so a load behind a store waits for it) and are in flight under the next chunk's
//     DMA wait and MFMAs;
//   * the x tiles [64 k][128] of a chunk arrive by LDS-DMA all at once -- one round trip per
//     chunk instead of one per tile, the measured lever (profiles/r7_fc_sgd_stream_probe.md; the
//     (64, 256), (32, 512) and (128, 128) shapes tried there were retired) -- into LDS shared with
//     the per-wave fp32 staging of the epilogue.
#include "gemm_glds_common.h"

using namespace cxg;

namespace {

constexpr int RJ = 64, CI = 128;         // the strip's rows, the chunk's columns
constexpr int SUB_BYTES = CI * BK * 2;   // one MN-major [64 k][128 columns] bf16 image
constexpr int EP_PITCH = CI + 4;         // floats per staged row
constexpr int NS = 8;                    // slots per chunk: wave instructions of 2 rows x 128 columns
// NKT 64-k tiles are held (K <= 64 NKT): 4 at 2 blocks per CU; 8 hold twice the dy fragments and x
// tiles and run 1 block per CU
constexpr int blocks_per_cu(int nkt) { return nkt <= 4 ? 2 : 1; }
static_assert(4 * 16 * EP_PITCH * 4 <= 4 * SUB_BYTES, "the staging fits the x tiles' LDS");
static_assert(2 * 4 * SUB_BYTES <= 160 * 1024 && 8 * SUB_BYTES <= 160 * 1024, "LDS");

// Work items = (strip, chunk) pairs, strip-major; block b of nb takes items [b n / nb, (b + 1) n / nb):
// equal shares whatever the shape.  A share that crosses into the next strip reloads the dy
// fragments there.
template <int NKT>
__global__ void __launch_bounds__(256, (blocks_per_cu(NKT)))
fc_wgrad_sgd_stream(GOperand A, GOperand B, GEpi E, int nchunks, int items, int ktiles) {
  using OX = Op<MN_DIRECT, 128, 4>;
  __shared__ __attribute__((aligned(1024))) char smem[NKT * SUB_BYTES];

  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);  // rows 16 wave .. of the strip
  const rsrc_t rA = make_rsrc(A.ptr, A.nbytes);
  const rsrc_t rB = make_rsrc(B.ptr, B.nbytes);
  const int Mi = A.rows, Nj = B.rows;
  SgdHyp hy = {E.lr, E.wd, E.mom, E.clip};  // as sgd_hyper: the device array wins when given
  if (const float *hp = E.sgd_hyp) hy = {hp[0], hp[1], hp[2], hp[3]};
  int item = static_cast<int>(static_cast<long>(blockIdx.x) * items / gridDim.x);
  const int item_end = static_cast<int>((static_cast<long>(blockIdx.x) + 1) * items / gridDim.x);
  // slot s = rows 2 s, 2 s + 1 of the wave: 32 lanes per row, 16 bytes each
  const int il = (lane & 31) * 4;
  float *ep = reinterpret_cast<float *>(smem) + wave * 16 * EP_PITCH;

  while (item < item_end) {  // one run of chunks of one strip
    const int strip = item / nchunks;
    const int c_beg = item - strip * nchunks;
    const int c_end = min(nchunks, c_beg + (item_end - item));
    item += c_end - c_beg;
    const int j0 = strip * RJ;

    // ---- the strip's dy fragments: [64 k][128 j] images through LDS
    bf16x8 fb[NKT][2];
    {
      OX ob;
      ob.init(B, j0, 0u, wave, lane);
      static_for<NKT>([&](auto tc) {
        constexpr int t = decltype(tc)::value;
        if (t < ktiles) {
          const typename OX::Prep pb = ob.prep(B, t, ktiles, 0u);
          static_for<OX::NI>([&](auto sc) {
            constexpr int s = decltype(sc)::value;
            __builtin_amdgcn_raw_ptr_buffer_load_lds(rB, (lds_void *)(smem + t * SUB_BYTES + (wave + 4 * s) * 1024),
                                                     16, ob.template offset<s>(B, pb, wave, lane), 0, 0, 0);
          });
        }
      });
      wait_vmcnt<0>();
      __syncthreads();
      static_for<NKT>([&](auto tc) {
        constexpr int t = decltype(tc)::value;
        fb[t][0] = fb[t][1] = bf16x8{0, 0, 0, 0, 0, 0, 0, 0};
        if (t < ktiles) {
          fb[t][0] = frag<MN_DIRECT>(smem + t * SUB_BYTES, wave * 16, 0, lane);
          fb[t][1] = frag<MN_DIRECT>(smem + t * SUB_BYTES, wave * 16, 32, lane);
        }
      });
      __syncthreads();
    }

    const int jlane = j0 + wave * 16 + (lane >> 5);
    f32x4 pw[NS], pm[NS];
#pragma unroll
    for (int q = 0; q < NS; ++q) pw[q] = pm[q] = f32x4{0.f, 0.f, 0.f, 0.f};
    // the w / m loads of slot s of chunk cc (lanes outside the matrix keep what they hold)
    auto load_slot = [&](int cc, int s, f32x4 &wv, f32x4 &mv) {
      const int j = jlane + 2 * s;
      const int i = cc * CI + il;
      if (j < Nj && i < Mi) {
        const long idx = static_cast<long>(j) * E.ldc + i;
        wv = *reinterpret_cast<const f32x4 *>(E.sgd_w + idx);
        mv = *reinterpret_cast<const f32x4 *>(E.sgd_m + idx);
      }
    };
    static_for<NS>([&](auto sc) {
      constexpr int s = decltype(sc)::value;
      load_slot(c_beg, s, pw[s], pm[s]);
    });

    for (int c = c_beg; c < c_end; ++c) {
      const int i0 = c * CI;
      OX oa;
      oa.init(A, i0, 0u, wave, lane);
      f32x4 acc[8];
#pragma unroll
      for (int m = 0; m < 8; ++m) acc[m] = f32x4{0.f, 0.f, 0.f, 0.f};

      // ---- the chunk's GEMM: every x tile in one DMA round trip
      static_for<NKT>([&](auto tc) {
        constexpr int t = decltype(tc)::value;
        if (t < ktiles) {
          const typename OX::Prep pa = oa.prep(A, t, ktiles, 0u);
          static_for<OX::NI>([&](auto sc) {
            constexpr int s = decltype(sc)::value;
            __builtin_amdgcn_raw_ptr_buffer_load_lds(rA, (lds_void *)(smem + t * SUB_BYTES + (wave + 4 * s) * 1024),
                                                     16, oa.template offset<s>(A, pa, wave, lane), 0, 0, 0);
          });
        }
      });
      wait_vmcnt<0>();
      block_barrier();
      static_for<NKT>([&](auto tc) {
        constexpr int t = decltype(tc)::value;
        if (t < ktiles) {
          static_for<2>([&](auto hc) {
            constexpr int h = decltype(hc)::value;
#pragma unroll
            for (int m = 0; m < 8; ++m) {
              const bf16x8 fa = frag<MN_DIRECT>(smem + t * SUB_BYTES, m * 16, h * 32, lane);
              acc[m] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(fa, fb[t][h], acc[m], 0, 0, 0);
            }
          });
        }
      });
      __syncthreads();  // the x tiles' LDS is reused by the staging

      // ---- the chunk's stream: stage the wave's 16 rows, then per slot: update, load the next
      // chunk's slot, store
#pragma unroll
      for (int m = 0; m < 8; ++m)
        *reinterpret_cast<f32x4 *>(ep + (lane & 15) * EP_PITCH + m * 16 + (lane >> 4) * 4) = acc[m];
      __builtin_amdgcn_s_waitcnt(0xc07f);  // lgkmcnt(0)
      wave_lds_handoff<true>();
      static_for<NS>([&](auto sc) {
        constexpr int s = decltype(sc)::value;
        const int jl = (lane >> 5) + 2 * s;
        const int j = jlane + 2 * s;
        const int i = i0 + il;
        const bool ok = j < Nj && i < Mi;
        const long idx = static_cast<long>(j) * E.ldc + i;
        f32x4 w4 = pw[s], m4 = pm[s];
        if (ok) {
          const f32x4 v = *reinterpret_cast<const f32x4 *>(ep + jl * EP_PITCH + il) * E.alpha;
#pragma unroll
          for (int e = 0; e < 4; ++e) {
            float mm = m4[e];
            w4[e] = sgd_step(hy, v[e], mm, w4[e]);
            m4[e] = mm;
          }
        }
        if (c + 1 < c_end) load_slot(c + 1, s, pw[s], pm[s]);
        if (ok) {
          *reinterpret_cast<f32x4 *>(E.sgd_w + idx) = w4;
          *reinterpret_cast<f32x4 *>(E.sgd_m + idx) = m4;
          *reinterpret_cast<uint2 *>(E.sgd_wb + idx) = make_uint2(pack2(w4[0], w4[1]), pack2(w4[2], w4[3]));
        }
      });
      __builtin_amdgcn_s_waitcnt(0xc07f);
      wave_lds_handoff<true>();
      __syncthreads();  // the staging is overwritten by the next chunk's DMAs
    }
  }
}

int g_cus = 0;  // compute units of the device (queried once)

}  // namespace

namespace cxg {
// forced: serve every shape the kernel can (tests, probes); else decline shapes it does not pay
// for.  blocks > 0: that many blocks (at most one per item) instead of as many as the CUs hold.
// -1 when not served (the caller then takes the tile dispatch).  Served: K <= 512; nout, nin and
// K tails by guards and DMA zeros.
int dispatch_fc_sgd_stream(const GOperand &A, const GOperand &B, const GEpi &E, bool forced, int blocks_set,
                           hipStream_t s) {
  if (A.kdim > 8 * BK) return -1;
  if (g_cus <= 0) {
    int dev = 0, n = 0;
    if (hipGetDevice(&dev) != hipSuccess || hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess)
      n = 256;
    g_cus = n > 0 ? n : 256;
  }
  const int strips = cdiv(B.rows, RJ), nchunks = cdiv(A.rows, CI), ktiles = cdiv(A.kdim, BK);
  const long items = static_cast<long>(strips) * nchunks;
  if (items >= (1L << 31)) return -1;
  // as many blocks as the CUs hold at once, each with an equal share of the items
  long blocks = static_cast<long>(blocks_per_cu(ktiles <= 4 ? 4 : 8)) * g_cus;
  // shares of fewer than 2 chunks carry nothing from chunk to chunk: the tile kernel's job
  if (!forced && items < 2 * blocks) return -1;
  if (blocks_set > 0) blocks = blocks_set;
  if (blocks > items) blocks = items;
  const dim3 grid(static_cast<uint32_t>(blocks));
  if (ktiles <= 4)
    CXN_LAUNCH((fc_wgrad_sgd_stream<4>), grid, dim3(256), 0, s, A, B, E, nchunks, static_cast<int>(items), ktiles);
  else
    CXN_LAUNCH((fc_wgrad_sgd_stream<8>), grid, dim3(256), 0, s, A, B, E, nchunks, static_cast<int>(items), ktiles);
  return 0;
}
}  // namespace cxg
