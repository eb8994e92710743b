// 256 x 256 x 64 bf16 GEMM kernel with direct-to-LDS operand loads, for every operand layout (Linear forward, dX, dW).
//
// Why: ablation of the 128 x 128 kernel (scripts/exp/ablate_gemm.hip) showed the per-CU vector-memory return path and the
// VGPR -> LDS store path each cost as many cycles per tile as the MFMAs.  Here operands never touch VGPRs on the way in:
//
//   * 8 waves (2 M x 4 N), wave tile 128 x 64 = 8 x 4 MFMA 16x16x32 fragments (128 accumulator VGPRs), one block per CU.
//   * Operand tiles arrive by LDS-DMA (`buffer_load_dwordx4 ... lds`, 1 KiB per wave-instruction, 8 per wave per K-tile)
//     into two 64 KiB stages.  The LDS image is lane-linear, so the bank swizzle is applied to the per-lane SOURCE offset:
//       k-contiguous operand: [256 rows][128 B]; 16-byte chunk c of row r sits at chunk (c ^ ((r >> 1) & 7))
//                             -> each 16-lane group of a ds_read_b128 fragment read covers all 64 banks once
//       k-major operand:      [64 k-rows][512 B]; chunk c of k-row k sits at chunk (c ^ (s(k) << 1)), s(k) = k[1:0] | k[3] << 2
//                             -> the 8 k-rows one half-wave of ds_read_b64_tr_b16 touches fall on 8 distinct 32-byte bank slots
//     Rows outside the matrix and k beyond K are redirected to an out-of-range buffer offset (hardware returns zeros).
//   * K loop, software-pipelined inside each wave (fragment registers double-buffered, reads issued by inline asm so the
//     waits are counted by hand):  the ks=1 fragment reads run under the ks=0 MFMAs; then `vmcnt(0) lgkmcnt(0)` + ONE raw
//     s_barrier per K-tile; right after it the fragment reads of tile t+1 begin under the last MFMAs of tile t, and the DMA pieces
//     of tile t+2 go into the stage just drained one per MFMA group (Ring).  The DMA has a whole K-tile of MFMA time
//     (>= 2048 cycles) to land.
//   * Epilogue: alpha / bias / rowvec / GELU in registers, C staged through LDS in row passes, 16-byte row-contiguous
//     global stores with residual / accumulate applied on the way out; split-K slices go to a workspace.
//
// One of each: Dma<L, BK> (operand DMA addressing, both K-tile widths), Frags<L, NF, BK> / frag_read (LDS -> MFMA fragments), Ring
// (wait arithmetic, fragment reads, MFMA step and DMA spreading of the 64-wide K loop, shared with gemm256p.h), xcd_tile_index /
// raster_origin (tile order).  The pipes - Pipe (64-wide, two stages), Pipe32 (32-wide, five stages), PipeX3 (four-plane bf16x3) -
// have one interface (prologue, ktile<stage>, drain; da / db / fa / fb); tile_body is tile and K-range set-up, the K loop over that
// interface, and the epilogue.  Host side (cost model, launchers): gemm256_host.h; eligibility (gemm256_ok): gemm_p.h.
//
// How far the sharing goes is set by the compiler's output (scripts/kernel_digest.py, profiles/gemm256_refactor_isa.md): every kernel
// compiles to the instruction stream it had before this code was shared.  These kernels sit at
// 256 VGPRs with a few bytes of scratch, and hipcc simplifies every function on its own before it inlines it, so a new function level
// around set-up arithmetic, the K loop, the epilogue or the DMA builtin changes operand order, spills or the loop guard.  That is why
// tile_body keeps the K loop and the epilogue in its own body, why the pipes' set-up is spelled out there, why Dma::init writes each
// tile format's geometry out, why Ring holds no data, and why g256p::DmaP and g256p::Sched::decode restate what Dma::init,
// xcd_tile_index and raster_origin say: a change to a swizzle or to the tile order is made there as well.
#pragma once
#include "gemm_core.h"
#include <type_traits>

namespace g256 {

typedef __attribute__((address_space(3))) void lds_void_t;
constexpr int BM = 256, BN = 256, BK = 64, NT = 512, MI = 8, NI = 4;
constexpr int TILE = 32768;                 // one operand tile of one stage
constexpr int A_BASE = 0, B_BASE = 65536;   // stage s of an operand at BASE + s * TILE
constexpr int LDS_BYTES = 131072;

// swizzles: k-major tiles (either K-tile width); 64-byte rows of the 32-wide k-contiguous tile
__device__ __forceinline__ int km_sw(int kr) { return (kr & 3) | (((kr >> 3) & 1) << 2); }
__device__ __forceinline__ int sw4(int q) { return (4 - q) & 3; }

template <int OFF> __device__ __forceinline__ void lds_read128(bf16x8& d, unsigned addr) {
  asm volatile("ds_read_b128 %0, %1 offset:%2" : "=v"(d) : "v"(addr), "n"(OFF));
}
template <int OFF> __device__ __forceinline__ void lds_read64_tr(u32x2& d, unsigned addr) {
  asm volatile("ds_read_b64_tr_b16 %0, %1 offset:%2" : "=v"(d) : "v"(addr), "n"(OFF));
}
// One MFMA of the K loop: bf16 operands, or (H) the same 16-bit lanes read as IEEE half - 11 significant bits per operand, the TF32
// operand precision, at the bf16 rate (gfx950 has no xf32 MFMA); fragments, LDS images and DMA are the same bytes either way.
typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));
template <bool H> __device__ __forceinline__ f32x4 mfma16(const bf16x8& a, const bf16x8& b, const f32x4& c) {
#ifdef G256_ABLATE_NO_MFMA   // timing experiment (scripts/exp/ablate256.sh): the operands stay live, no MFMA is issued - in every pipe (PipeX3 and
  // g256p::PipeP too, which the macro did not reach when profiles/r06_gemm256_ablation.txt was taken; one liveness statement per MFMA, not per group)
  asm volatile("" ::"v"(a), "v"(b)); return c;
#else
  if constexpr (H) return __builtin_amdgcn_mfma_f32_16x16x32_f16(__builtin_bit_cast(f16x8, a), __builtin_bit_cast(f16x8, b), c, 0, 0, 0);
  else return __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, b, c, 0, 0, 0);
#endif
}
template <int N> __device__ __forceinline__ void wait_lgkm() {
  asm volatile("s_waitcnt lgkmcnt(%0)" ::"n"(N) : "memory");
  __builtin_amdgcn_sched_barrier(0);
}
#ifdef G256_TIMESTAMPS   // timing experiments (scripts/exp/gemm_ts.py): s_memtime stamps per block - 0 entry, 1 prologue done, 2 K loop done, 3 exit
__device__ long* g_gemm_ts = nullptr;
#define G256_TS(IDX) if (g_gemm_ts && threadIdx.x == 0 && blockIdx.y == 0 && blockIdx.z == 0) g_gemm_ts[(long)blockIdx.x * 4 + (IDX)] = (long)__builtin_amdgcn_s_memtime();
#else
#define G256_TS(IDX)
#endif

// ---- tile order ------------------------------------------------------------------------------------------------------------------
// XCD swizzle: workgroup b runs on XCD b & 7; XCD x walks a contiguous range of the tile list (8 bq + br tiles: bq + 1 each for the
// first br XCDs, bq for the rest), so that the tiles in flight on one XCD share their operand panels in that XCD's L2.  -> this
// workgroup's tile.  (g256p::Sched::decode walks the same ranges from a queue position, with bq / br computed by the host.)
__device__ __forceinline__ int xcd_tile_index(int ntiles) {
  const int bq = ntiles >> 3, br = ntiles & 7, xcd = blockIdx.x & 7, bi = blockIdx.x >> 3;
  return (xcd < br ? xcd * (bq + 1) : br * (bq + 1) + (xcd - br) * bq) + bi;
}
// grouped raster: tile `id` of ntm x ntn tiles -> origin; groups of GM = 4 row tiles are walked column by column
__device__ __forceinline__ void raster_origin(int id, int ntm, int ntn, int& m0, int& n0) {
  constexpr int GM = 4;
  const int grp = id / (GM * ntn), first_m = grp * GM;
  const int gm = min(ntm - first_m, GM), in_grp = id - grp * (GM * ntn);
  m0 = (first_m + in_grp % gm) * BM;
  n0 = (in_grp / gm) * BN;
}

// ---- LDS-DMA of one operand (256 rows x BK k) --------------------------------------------------------------------------------------
// Each wave issues NP = BK / 16 pieces of 1 KiB per K-tile; piece q = wave * NP + j lands at tile + q * 1024 (+ lane * 16 by hardware).
// A piece is 8 rows of 128 B (k-contiguous, BK = 64), 16 rows of 64 B (k-contiguous, BK = 32) or 2 k-rows of 512 B (k-major).
template <int L, int BK>
struct Dma {
  static constexpr int NP = BK / 16;
  rsrc_t rs;
  unsigned voff[NP];  // byte offset of this lane's chunk of piece j at K-tile 0 (or `oob`)
  unsigned kk0;       // k (inside the tile) of this lane's chunk of piece 0
  unsigned oob;
  unsigned kstep;     // bytes per K-tile
  int kend;
  // a tile whose first row (k-contiguous) / column (k-major) is r0; rows / columns from R on are redirected out of range
  __device__ __forceinline__ void init(const bf16_t* ptr, long ld, int R, int K, int kend_, int r0, int wave, int lane) {
    kend = kend_;
    const long cols = L == 0 ? K : R, rows = L == 0 ? R : K;
    const unsigned bytes = (unsigned)(((rows - 1) * ld + (cols + 7) / 8 * 8) * 2);
    rs = make_rsrc(ptr, bytes);
    oob = (bytes + 15u) & ~15u;
    if constexpr (L == 0 && BK == 64) {
      const int r8 = lane >> 3, pc = lane & 7;
      kstep = 128u;
      kk0 = (unsigned)((pc ^ (r8 >> 1)) * 8);
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int row = (wave * 4 + j) * 8 + r8;           // (row >> 1) & 7 == ((j & 1) << 2) | (r8 >> 1)
        const int csrc = pc ^ ((row >> 1) & 7);
        voff[j] = (r0 + row) < R ? (unsigned)(((long)(r0 + row) * ld + csrc * 8) * 2) : oob;
      }
    } else if constexpr (L == 0) {
      const int csrc = (lane & 3) ^ sw4((lane >> 4) & 3);
      kstep = 64u;
      kk0 = (unsigned)(csrc * 8);
#pragma unroll
      for (int j = 0; j < 2; ++j) {
        const int row = (wave * 2 + j) * 16 + (lane >> 2);
        voff[j] = (r0 + row) < R ? (unsigned)(((long)(r0 + row) * ld + csrc * 8) * 2) : oob;
      }
    } else {
      const int half = lane >> 5, pos = lane & 31;
      kstep = (unsigned)(BK * ld * 2);
      kk0 = (unsigned)(wave * (2 * NP) + half);
#pragma unroll
      for (int j = 0; j < NP; ++j) {
        const int kr = wave * (2 * NP) + j * 2 + half;
        const int csrc = pos ^ (km_sw(kr) << 1);
        voff[j] = (r0 + csrc * 8) < R ? (unsigned)(((long)kr * ld + r0 + csrc * 8) * 2) : oob;
      }
    }
  }
  // k of this lane's chunk of piece j inside its tile
  __device__ __forceinline__ unsigned kk(int j) const {
    return L == 1 ? (kk0 + 2u * j) : BK == 64 ? (kk0 ^ ((unsigned)(j & 1) << 5)) : kk0;
  }
  // piece J of tile kt alone -> LDS byte offset `lds_off` (stage base + operand base; wave-uniform).  A tile at or beyond kend is all
  // out-of-range chunks: zeros, no memory traffic
  template <int J>
  __device__ __forceinline__ void issue1(unsigned char* smem, int lds_off, int kt, int wave) const {
    const unsigned vo = ((unsigned)kt * (unsigned)BK + kk(J)) < (unsigned)kend ? voff[J] : oob;
    __builtin_amdgcn_raw_ptr_buffer_load_lds(rs, (lds_void_t*)(smem + lds_off + (wave * NP + J) * 1024), 16, (int)vo, (int)((unsigned)kt * kstep), 0, 0);
  }
  __device__ __forceinline__ void issue(unsigned char* smem, int lds_off, int kt, int wave) const {
    const unsigned soff = (unsigned)kt * kstep;
#pragma unroll
    for (int j = 0; j < NP; ++j) {
      const unsigned vo = ((unsigned)kt * (unsigned)BK + kk(j)) < (unsigned)kend ? voff[j] : oob;
      __builtin_amdgcn_raw_ptr_buffer_load_lds(rs, (lds_void_t*)(smem + lds_off + (wave * NP + j) * 1024), 16, (int)vo, (int)soff, 0, 0);
    }
  }
};

// ---- LDS -> MFMA fragments of one operand: NF fragments of 16 rows; lane supplies row (lane & 15), k = 8 * (lane >> 4) .. +7 ---
// one fragment at addr + OFF: a 128-bit read (k-contiguous tile) or a transposed pair, repacked (k-major tile)
template <int L, int OFF> __device__ __forceinline__ void frag_read(bf16x8& d, unsigned addr) {
  if constexpr (L == 0) {
    lds_read128<OFF>(d, addr);
  } else {
    u32x2 h0, h1;
    lds_read64_tr<OFF>(h0, addr);
    lds_read64_tr<OFF + 2048>(h1, addr);
    const u32x4 w = {h0[0], h0[1], h1[0], h1[1]};
    d = __builtin_bit_cast(bf16x8, w);
  }
}
template <int L, int NF, int BK>
struct Frags {
  static constexpr int PITCH = 2 * BK;                      // bytes per row of a k-contiguous tile
  static constexpr int NADDR = L == 0 ? BK / 32 : NF;       // one address per K-group (k-contiguous) / per fragment (k-major)
  static constexpr int READS_PER_FRAG = L == 0 ? 1 : 2;
  unsigned addr[NADDR];
  __device__ __forceinline__ void init(int base, int wb, int lane) {
    const int p = lane & 15, g = lane >> 4;
    if constexpr (L == 0) {
      const int sw = BK == 64 ? (p >> 1) & 7 : sw4((p >> 2) & 3);
#pragma unroll
      for (int ks = 0; ks < NADDR; ++ks) addr[ks] = (unsigned)(base + (wb + p) * PITCH + (((ks * 4 + g) ^ sw) << 4));
    } else {
      const int kr = 8 * g + (p >> 2), s = km_sw(kr);
#pragma unroll
      for (int f = 0; f < NF; ++f) {
        const int chunk = (wb >> 3) + 2 * f + ((p & 3) >> 1);
        addr[f] = (unsigned)(base + kr * 512 + ((chunk ^ (s << 1)) << 4) + (p & 1) * 8);
      }
    }
  }
  // the fragments of `base`, `off` bytes further (another stage)
  __device__ __forceinline__ void point_at(const Frags& base, unsigned off) {
#pragma unroll
    for (int f = 0; f < NADDR; ++f) addr[f] = base.addr[f] + off;
  }
  // fragment F of K-group KS, OFF bytes beyond the tile `init` pointed at
  template <int OFF, int KS, int F>
  __device__ __forceinline__ void read(bf16x8& d) const {
    if constexpr (L == 0) frag_read<0, OFF + F * 16 * PITCH>(d, addr[KS]);
    else frag_read<1, OFF + KS * 16384>(d, addr[F]);
  }
  template <int OFF, int KS, int F0, int F1>
  __device__ __forceinline__ void read_range(bf16x8 (&d)[NF]) const {
    if constexpr (F0 < F1) {
      read<OFF, KS, F0>(d[F0]);
      read_range<OFF, KS, F0 + 1, F1>(d);
    }
  }
};

// ---- the K loop: one wave's view ----------------------------------------------------------------------------------------
// A K-tile is 16 MFMA "groups" g = ks * 8 + i (the 4 MFMAs of A-fragment row i against the 4 B fragments of K-group ks).
// A fragments live in a ring of NSLOT registers and are read DIST groups ahead of their use; the B fragments of both
// K-groups stay resident (read once per tile: ks=1 at group GB1, the next tile's ks=0 at group GBAR, right after the
// barrier).  The barrier sits before group GBAR = 16 - DIST, the first group whose look-ahead read targets the next stage:
//   wait vmcnt(0) lgkmcnt(0)   my DMA pieces of tile t+1 have landed, my reads of this stage are complete
//   s_barrier                  ... and so have everyone's
//   DMA tile t+2 -> this stage; fragment reads of tile t+1 begin, under the last DIST groups of MFMAs of tile t.
// LDS reads return in order, so "fragment a(g) has arrived" == at most (reads issued after it) outstanding: ring_wait.
//
// The 8 DMA pieces of a tile are not issued in one burst behind the barrier but one per MFMA group (`spread`) - pieces 0..2 of tile
// t+2 in groups 13..15 of tile t (its stage is free from the barrier on), pieces 3..7 in groups 0..4 of tile t+1.  A burst of 8
// pieces costs each wave ~150 cycles of issue per piece with both waves of the SIMD doing the same thing at the same time
// (MI355X_MICROARCH.md: "LDS-DMA piece issue cost"); a single piece among MFMAs costs ~60 and the partner wave's MFMAs run under it.
// MI355X, [16448x768]x[6144x768]^T and its dX / dW, burst -> spread: 874 -> 920, 873 -> 970, 869 -> 955 TFLOP/s; bit-identical.
// Tried on top and dropped (profiles/r06_gemm256_ablation.txt): all eight pieces in the three groups behind the barrier, two per
// group, and an L2 touch-prefetch of the tiles a few K-tiles ahead.
//
// lgkmcnt when group g needs its A fragment: the DIST look-ahead reads (RA instructions each) behind it, plus the B reads (NB
// instructions at groups GB1 and GBAR of every PERIOD groups) issued among them; the counter holds 15 at most
constexpr int ring_wait(int g, int PERIOD, int DIST, int RA, int NB, int GB1, int GBAR) {
  int n = DIST * RA;
  for (int x = g - DIST + 1; x <= g; ++x) {
    const int xm = ((x % PERIOD) + PERIOD) % PERIOD;
    n += (xm == GB1 || xm == GBAR) ? NB : 0;
  }
  return n > 15 ? 15 : n;
}

// Waits and per-group steps of the 64-wide K loop, for the launch-per-tile schedule (Pipe) and the persistent one (g256p::PipeP).
// A base without data: the pipe P itself declares da, db, fa, fb, acc, ring, bk, smem, wave - with them in a base sub-object hipcc
// compiled the persistent kernels differently (profiles/gemm256_refactor_isa.md).
template <class P, int AL, int BL, bool H>
struct Ring {
  static constexpr int RA = AL ? 2 : 1, RB = BL ? 2 : 1, NB = NI * RB;
  static constexpr int NSLOT = 4, DIST = NSLOT - 1;
  static constexpr int GB1 = 8 - DIST, GBAR = 16 - DIST;
  __device__ __forceinline__ P& me() { return *static_cast<P*>(this); }

  static constexpr int waitN(int g) { return ring_wait(g, 16, DIST, RA, NB, GB1, GBAR); }
  // A fragment of virtual group GA: 0..15 = this tile (stage S), 16.. = next tile (stage S ^ 1)
  template <int S, int GA>
  __device__ __forceinline__ void read_a() {
    constexpr int st = GA < 16 ? S : (S ^ 1), g = GA & 15;
    me().fa.template read<st * TILE, (g >> 3), (g & 7)>(me().ring[GA & (NSLOT - 1)]);
  }
  // DMA piece Q (0..3 of A, 4..7 of B) of tile kt -> stage STAGE
  template <int STAGE, int Q>
  __device__ __forceinline__ void issue_piece(int kt) {
    if constexpr (Q < 4) me().da.template issue1<Q>(me().smem, A_BASE + STAGE * TILE, kt, me().wave);
    else me().db.template issue1<Q - 4>(me().smem, B_BASE + STAGE * TILE, kt, me().wave);
  }
  // the piece that goes out in group G of tile kt (stage S).  HEAD = false: none in groups 0..4 (the persistent kernel's tile change
  // has issued pieces 3..7 already).  Tiles at or beyond kend are zero-fill pieces: the piece count per tile stays uniform for the waits
  template <int S, int G, bool HEAD = true>
  __device__ __forceinline__ void spread(int kt) {
    if constexpr (G >= GBAR) issue_piece<S, G - GBAR>(kt + 2);
    else if constexpr (G < 8 - (16 - GBAR) && HEAD) issue_piece<S ^ 1, G + (16 - GBAR)>(kt + 1);
  }
  template <int G> __device__ __forceinline__ void prologue_a() {
    if constexpr (G < DIST) { read_a<0, G>(); prologue_a<G + 1>(); }
  }
  // behind the first barrier: the B fragments of K-group 0 and the first DIST A fragments of the tile in stage 0
  __device__ __forceinline__ void prime() {
    me().fb.template read_range<0, 0, 0, NI>(me().bk[0]);
    prologue_a<0>();
    __builtin_amdgcn_sched_barrier(0);
  }
  // behind the barrier of group GBAR: the next tile's B fragments of K-group 0 (after the last tile: a stale stage, never used)
  template <int S> __device__ __forceinline__ void read_b_next() { me().fb.template read_range<(S ^ 1) * TILE, 0, 0, NI>(me().bk[0]); }
  // fragment reads and MFMAs of group G of the tile in stage S
  template <int S, int G>
  __device__ __forceinline__ void step() {
    if constexpr (G == GB1) me().fb.template read_range<S * TILE, 1, 0, NI>(me().bk[1]);
    read_a<S, G + DIST>();
    wait_lgkm<waitN(G)>();
#pragma unroll
    for (int j = 0; j < NI; ++j)
      me().acc[G & 7][j] = mfma16<H>(me().bk[G >> 3][j], me().ring[G & (NSLOT - 1)], me().acc[G & 7][j]);
    __builtin_amdgcn_sched_barrier(0);
  }
};

// Every pipe has da / db (X3: and dal / dbl, the lo planes) and fa / fb at FA_BASE / FB_BASE for tile_body to set up, and runs K-tiles
// [kt0, kt_last) - an even count: a tile beyond kend is all out-of-range chunks - as prologue, ktile<stage> per K-tile, drain (trailing waits).
// One call shape for tile_body; what each pipe uses of it: Pipe prologue(kt0), ktile(kt); Pipe32 prologue(kt0), ktile() - it counts its
// tiles itself (kt_issue); PipeX3 both arguments of both (it issues no DMA piece for a tile at or beyond kt_last).
template <int AL, int BL, bool H = false>
struct Pipe : Ring<Pipe<AL, BL, H>, AL, BL, H> {
  using R = Ring<Pipe<AL, BL, H>, AL, BL, H>;
  using R::GBAR; using R::NSLOT;
  Dma<AL, 64> da;
  Dma<BL, 64> db;
  Frags<AL, MI, 64> fa;
  Frags<BL, NI, 64> fb;
  f32x4 acc[MI][NI];
  bf16x8 ring[NSLOT];
  bf16x8 bk[2][NI];
  unsigned char* smem;
  int wave;
  static constexpr int BK = 64, FA_BASE = A_BASE, FB_BASE = B_BASE;
  static constexpr bool X3 = false;

  // K-tile kt, in stage S: its 16 MFMA groups from G on
  template <int S, int G = 0>
  __device__ __forceinline__ void ktile(int kt, int kt_last) {
    if constexpr (G == GBAR) {
      asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");
      __builtin_amdgcn_s_barrier();
      __builtin_amdgcn_sched_barrier(0);
      this->template read_b_next<S>();
    }
#ifndef G256_ABLATE_NO_DMA   // timing experiment (scripts/exp/ablate256.sh): no DMA inside the K loop
    this->template spread<S, G>(kt);
#endif
    this->template step<S, G>();
    if constexpr (G + 1 < 16) ktile<S, G + 1>(kt, kt_last);
  }
  __device__ __forceinline__ void prologue(int kt0, int) {
    da.issue(smem, A_BASE, kt0, wave);
    db.issue(smem, B_BASE, kt0, wave);
    // pieces 3..7 of the second tile follow in groups 0..4 of the first
    this->template issue_piece<1, 0>(kt0 + 1); this->template issue_piece<1, 1>(kt0 + 1); this->template issue_piece<1, 2>(kt0 + 1);
    asm volatile("s_waitcnt vmcnt(3)" ::: "memory");
    __builtin_amdgcn_s_barrier();
    __builtin_amdgcn_sched_barrier(0);
    this->prime();
  }
  __device__ __forceinline__ void drain() {
    wait_lgkm<0>();  // the trailing (unused) fragment reads must not land in registers the epilogue reuses
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");   // ... nor the trailing zero-fill DMA pieces in the LDS bytes the epilogue stages C in
    __builtin_amdgcn_sched_barrier(0);
  }
};

// =====================================================================================================================
// BK = 32 variant with five 32 KiB stages (160 KiB of LDS): three K-tiles of DMA in flight instead of one.
// Ablation of the BK = 64 / 2-stage pipeline (scripts/exp/ablate256.sh, [16384x3072]x[6144x3072]^T): 594 us full,
// 467 us without the in-loop DMA, 342 us without the MFMAs, 153 us with neither - the DMA stream alone runs at 1.19 us per
// 64-wide K-tile although its bytes need 0.52 us of the CU's vector-memory path: with one stage in flight it is bound by
// issue -> landed latency (Little: 64 KiB in flight per CU vs ~75 KiB needed at MFMA speed).  Same wave tiling, same
// ring, same waits; per K-tile: 8 MFMA groups, barrier before group 5, `vmcnt(8)` (tiles t+2, t+3 stay in flight).
// 64-byte LDS rows for k-contiguous operands: chunk c of row r at chunk c ^ s4((r >> 2) & 3), s4 = {0,3,2,1}.
// =====================================================================================================================
constexpr int BK32 = 32, NST32 = 5, TILE32 = 16384, STAGE32 = 32768, LDS_BYTES32 = NST32 * STAGE32;

template <int AL, int BL>
struct Pipe32 {
  static constexpr int BK = 32, FA_BASE = 0, FB_BASE = 0;
  static constexpr bool X3 = false;
  static constexpr int RA = AL ? 2 : 1, RB = BL ? 2 : 1, NB = NI * RB;
  static constexpr int NSLOT = 4, DIST = NSLOT - 1, GBAR = 8 - DIST;
  Dma<AL, 32> da;
  Dma<BL, 32> db;
  Frags<AL, MI, 32> fa, fac;   // stage-0 addresses; addresses in the stage being read
  Frags<BL, NI, 32> fb, fbc;
  f32x4 acc[MI][NI];
  bf16x8 ring[NSLOT];
  bf16x8 bk[2][NI];
  unsigned char* smem;
  int wave;
  int so_next, so_issue, kt_issue;   // stage byte offsets of tile t+1 / of the next tile to DMA, and that tile's index

  static constexpr int waitN(int g) { return ring_wait(g, 8, DIST, RA, NB, GBAR, GBAR); }
  template <int G> __device__ __forceinline__ void prologue_a() {
    if constexpr (G < DIST) { fac.template read<0, 0, G>(ring[G]); prologue_a<G + 1>(); }
  }
  __device__ __forceinline__ void issue_next() {
    da.issue(smem, so_issue, kt_issue, wave);
    db.issue(smem, so_issue + TILE32, kt_issue, wave);
    so_issue = so_issue + STAGE32 == LDS_BYTES32 ? 0 : so_issue + STAGE32;
    ++kt_issue;
  }
  // one K-tile whose B fragments sit in bk[P]: its 8 MFMA groups (A fragment rows) from G on.  (The tile index lives in kt_issue.)
  template <int P, int G = 0>
  __device__ __forceinline__ void ktile(int kt, int kt_last) {
    if constexpr (G == GBAR) {
      asm volatile("s_waitcnt vmcnt(8) lgkmcnt(0)" ::: "memory");  // tile t+1 landed (t+2, t+3 in flight); my reads of tile t done
      __builtin_amdgcn_s_barrier();
      __builtin_amdgcn_sched_barrier(0);
      issue_next();                                  // tile t+4 -> the stage tile t-1 used
      fac.point_at(fa, (unsigned)so_next);
      fbc.point_at(fb, (unsigned)(so_next + TILE32));
      so_next = so_next + STAGE32 == LDS_BYTES32 ? 0 : so_next + STAGE32;
      fbc.template read_range<0, 0, 0, NI>(bk[P ^ 1]);
    }
    fac.template read<0, 0, ((G + DIST) & 7)>(ring[(G + DIST) & (NSLOT - 1)]);
    wait_lgkm<waitN(G)>();
#pragma unroll
    for (int j = 0; j < NI; ++j) acc[G][j] = mfma16<false>(bk[P][j], ring[G & (NSLOT - 1)], acc[G][j]);
    __builtin_amdgcn_sched_barrier(0);
    if constexpr (G + 1 < 8) ktile<P, G + 1>(kt, kt_last);
  }
  __device__ __forceinline__ void prologue(int kt0, int) {
    so_issue = 0; kt_issue = kt0;
    issue_next(); issue_next(); issue_next(); issue_next();
    so_next = STAGE32;
    asm volatile("s_waitcnt vmcnt(12)" ::: "memory");
    __builtin_amdgcn_s_barrier();
    __builtin_amdgcn_sched_barrier(0);
    fac.point_at(fa, 0u);
    fbc.point_at(fb, (unsigned)TILE32);
    fbc.template read_range<0, 0, 0, NI>(bk[0]);
    prologue_a<0>();
    __builtin_amdgcn_sched_barrier(0);
  }
  __device__ __forceinline__ void drain() {
    asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");  // trailing zero-fill DMAs and look-ahead reads
    __builtin_amdgcn_sched_barrier(0);
  }
};

// =====================================================================================================================
// "bf16x3" K loop: C = A_hi B_hi + A_hi B_lo + A_lo B_hi from FOUR operand planes (A_hi, A_lo at A + a_lo elements, B_hi, B_lo at
// B + b_lo; same leading dimension), f32 accumulation - the f32-class product of the tape engines' "bf16x3" mode as one kernel.
// Why not the plain kernel over K-concatenated operands (hi | hi | lo) x (hi | lo | hi) (ops.split_cat3, rounds 4-5): that form moves
// SIX operand tiles through the LDS-DMA path for three products, and the K loop of this tiling is bound by exactly that path
// (~27 B/clk per CU sustained against 31.8 B/clk needed at MFMA speed).  Here a 32-wide K-tile brings its four
// planes in once (64 KiB per stage, two stages) and the waves run 3 x 32 = 96 MFMAs on them: 21 B/clk of DMA at MFMA speed, and
// each fragment read from LDS feeds 1.5 x as many MFMAs.  Tile formats, swizzles and fragment addressing are the BK = 32 pipeline's
// (Dma<L, 32> / Frags<L, NF, 32>); per A-fragment row i: reads (a_hi, a_lo) of row i + 1, then b_lo x a_hi, b_hi x a_lo, b_hi x a_hi
// over the four B fragments (small terms first; 4 independent accumulators between two MFMAs on the same one).  One barrier per K-tile,
// before the last row: all fragment reads of the stage are complete there (row 7's were issued during row 6), so the DMA of tile t + 2
// goes into it, and the next tile's B fragments and row-0 A fragments are read under row 7's MFMAs.
// =====================================================================================================================
constexpr int X3_STAGE = 4 * TILE32, LDS_BYTES_X3 = 2 * X3_STAGE;

template <int AL, int BL>
struct PipeX3 {
  static constexpr int BK = 32, FA_BASE = 0, FB_BASE = 2 * TILE32;
  static constexpr bool X3 = true;
  static constexpr int RA = AL ? 2 : 1, RB = BL ? 2 : 1;
  Dma<AL, 32> da, dal;         // hi and lo plane of A
  Dma<BL, 32> db, dbl;
  Frags<AL, MI, 32> fa, fac;   // plane 0 of A inside a stage (stage 0; the stage being read); the lo plane TILE32 bytes further
  Frags<BL, NI, 32> fb, fbc;   // B_hi at 2 * TILE32, B_lo at 3 * TILE32
  f32x4 acc[MI][NI];
  bf16x8 ah[2], al[2];
  bf16x8 bh[2][NI], bl[2][NI];
  unsigned char* smem;
  int wave;

  template <int I, int SLOT> __device__ __forceinline__ void read_a() {
    fac.template read<0, 0, I>(ah[SLOT]);
    fac.template read<TILE32, 0, I>(al[SLOT]);
  }
  template <int P, int J> __device__ __forceinline__ void read_b() {
    if constexpr (J < NI) {
      fbc.template read<0, 0, J>(bh[P][J]);
      fbc.template read<TILE32, 0, J>(bl[P][J]);
      read_b<P, J + 1>();
    }
  }
  __device__ __forceinline__ void issue_tile(int stage_off, int kt) {
    da.issue(smem, stage_off, kt, wave);
    dal.issue(smem, stage_off + TILE32, kt, wave);
    db.issue(smem, stage_off + 2 * TILE32, kt, wave);
    dbl.issue(smem, stage_off + 3 * TILE32, kt, wave);
  }
  // The 8 DMA pieces of a tile are not issued as a burst behind the barrier (both waves of a SIMD sit at the same barrier: ~150 cycles
  // of issue per piece with no MFMA under it, measured on the plain kernel - Ring::spread) but one between two MFMA loops: pieces 0..2 of
  // tile t+2 in row 7 of tile t (its stage is free from the barrier on), pieces 3..7 in rows 0 and 1 of tile t+1 - five rows (~1900
  // cycles) before the barrier that needs them.
  template <int Q>
  __device__ __forceinline__ void issue_piece(int stage_off, int kt, int kt_last) {
    if (kt < kt_last) {
      if constexpr (Q < 2) da.template issue1<Q>(smem, stage_off, kt, wave);
      else if constexpr (Q < 4) dal.template issue1<Q - 2>(smem, stage_off + TILE32, kt, wave);
      else if constexpr (Q < 6) db.template issue1<Q - 4>(smem, stage_off + 2 * TILE32, kt, wave);
      else dbl.template issue1<Q - 6>(smem, stage_off + 3 * TILE32, kt, wave);
    }
  }
  // behind MFMA loop LOOP (0..2) of row I of the tile kt in stage S
  template <int S, int I, int LOOP>
  __device__ __forceinline__ void spread(int kt, int kt_last) {
    if constexpr (I == MI - 1) issue_piece<LOOP>(S * X3_STAGE, kt + 2, kt_last);
    else if constexpr (I == 0) issue_piece<3 + LOOP>((S ^ 1) * X3_STAGE, kt + 1, kt_last);
    else if constexpr (I == 1 && LOOP < 2) issue_piece<6 + LOOP>((S ^ 1) * X3_STAGE, kt + 1, kt_last);
  }
  // K-tile kt, in stage S (its B fragments sit in bh[S] / bl[S]): its rows from I on
  template <int S, int I = 0>
  __device__ __forceinline__ void ktile(int kt, int kt_last) {
    if constexpr (I == MI - 1) {
      asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");   // tile t+1 has landed; every read of this stage is complete
      __builtin_amdgcn_s_barrier();
      __builtin_amdgcn_sched_barrier(0);
      fac.point_at(fa, (unsigned)((S ^ 1) * X3_STAGE));
      fbc.point_at(fb, (unsigned)((S ^ 1) * X3_STAGE));
      read_b<S ^ 1, 0>();                                           // (after the last tile: a stale stage, never used)
      read_a<0, 0>();
    } else {
      read_a<I + 1, (I + 1) & 1>();
      wait_lgkm<2 * RA>();
    }
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int j = 0; j < NI; ++j) acc[I][j] = mfma16<false>(bl[S][j], ah[I & 1], acc[I][j]);
    __builtin_amdgcn_sched_barrier(0);
    spread<S, I, 0>(kt, kt_last);
#pragma unroll
    for (int j = 0; j < NI; ++j) acc[I][j] = mfma16<false>(bh[S][j], al[I & 1], acc[I][j]);
    __builtin_amdgcn_sched_barrier(0);
    spread<S, I, 1>(kt, kt_last);
#pragma unroll
    for (int j = 0; j < NI; ++j) acc[I][j] = mfma16<false>(bh[S][j], ah[I & 1], acc[I][j]);
    __builtin_amdgcn_sched_barrier(0);
    spread<S, I, 2>(kt, kt_last);
    __builtin_amdgcn_sched_barrier(0);
    if constexpr (I + 1 < MI) ktile<S, I + 1>(kt, kt_last);
  }
  __device__ __forceinline__ void prologue(int kt0, int kt_last) {
    issue_tile(0, kt0);
    issue_piece<0>(X3_STAGE, kt0 + 1, kt_last);
    issue_piece<1>(X3_STAGE, kt0 + 1, kt_last);
    issue_piece<2>(X3_STAGE, kt0 + 1, kt_last);
    asm volatile("s_waitcnt vmcnt(3)" ::: "memory");
    __builtin_amdgcn_s_barrier();
    __builtin_amdgcn_sched_barrier(0);
    fac.point_at(fa, 0u);
    fbc.point_at(fb, 0u);
    read_b<0, 0>();
    read_a<0, 0>();
    __builtin_amdgcn_sched_barrier(0);
  }
  __device__ __forceinline__ void drain() {
    asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");  // the trailing look-ahead reads
    __builtin_amdgcn_sched_barrier(0);
  }
};

// one 256 x 256 output tile (or one K slice of it) on pipe PipeT: `tid_` = the tile's index in the problem's grouped raster
template <typename TC, typename PipeT>
__device__ __forceinline__ void tile_body(const GemmParams& p, const int tid_, unsigned char* smem) {
  // ---- the tile, its batch slice and its K range ----
  int m0, n0;
  raster_origin(tid_, (p.M + BM - 1) / BM, (p.N + BN - 1) / BN, m0, n0);

  const int z = blockIdx.z, zq = z / p.zdiv, zr = z - zq * p.zdiv;
  const bf16_t* Ap = (const bf16_t*)p.A + zq * p.sA0 + zr * p.sA1;
  const bf16_t* Bp = (const bf16_t*)p.B + zq * p.sB0 + zr * p.sB1;
  TC* Cp = (TC*)p.C + zq * p.sC0 + zr * p.sC1 + (p.split_k > 1 ? (long)blockIdx.y * p.split_stride : 0L);

  constexpr int BKc = PipeT::BK;
  int nk = (p.K + BKc - 1) / BKc, kt0 = 0;
  if (p.split_k > 1) {
    const int nk64 = (p.K + 63) / 64;                 // slices are cut on 64-wide boundaries for either pipeline
    const int per = (nk64 + p.split_k - 1) / p.split_k;
    if (blockIdx.y * per >= nk64) return;
    kt0 = blockIdx.y * per * (64 / BKc);
    nk = min(nk, (blockIdx.y + 1) * per * (64 / BKc));
  }
  const int kend = min(p.K, nk * BKc);
  const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);

  // ---- the K loop ----
  const int wr = (wave >> 2) * 128, wc = (wave & 3) * 64;
  PipeT pp;
  pp.smem = smem; pp.wave = wave;
  pp.da.init(Ap, p.lda, p.M, p.K, kend, m0, wave, lane);
  if constexpr (PipeT::X3) pp.dal.init(Ap + p.a_lo, p.lda, p.M, p.K, kend, m0, wave, lane);
  pp.db.init(Bp, p.ldb, p.N, p.K, kend, n0, wave, lane);
  if constexpr (PipeT::X3) pp.dbl.init(Bp + p.b_lo, p.ldb, p.N, p.K, kend, n0, wave, lane);
  pp.fa.init(PipeT::FA_BASE, wr, lane);
  pp.fb.init(PipeT::FB_BASE, wc, lane);
#pragma unroll
  for (int i = 0; i < MI; ++i)
#pragma unroll
    for (int j = 0; j < NI; ++j) pp.acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};
  // the tile count is rounded up to even (a tile beyond kend is all out-of-range chunks: zeros, no memory traffic)
  const int kt_last = kt0 + ((nk - kt0 + 1) & ~1);
  pp.prologue(kt0, kt_last);
  G256_TS(1)
  for (int kt = kt0; kt < kt_last; kt += 2) {
    pp.template ktile<0>(kt, kt_last);
    pp.template ktile<1>(kt + 1, kt_last);
  }
  pp.drain();
  G256_TS(2)

  auto& acc = pp.acc;
  // ---- epilogue: C staged through LDS, RPP rows per pass, 16-byte row-contiguous stores ----
  // lane holds C[m][n..n+3], m = m0 + wr + 16 i + (lane & 15), n = n0 + wc + 16 j + 4 (lane >> 4)
  // (kept small on purpose: 128 accumulator registers per lane make every per-element branch 128 copies of code, and a
  //  one-block-per-CU kernel cannot hide an instruction-cache-missing epilogue behind another block)
  // Loads and stores share the in-order vmcnt queue, so any load consumed after a store waits for that store's acknowledgement,
  // and __syncthreads() is a global-memory fence (vmcnt(0)) as well.  Hence: (1) everything that has to be READ - bias, row
  // vector and, for f32 outputs, the residual and the old C of an accumulating product - is folded into the accumulators in
  // fragment layout BEFORE the first store; (2) the staging passes synchronise with LDS-only barriers.  (A bf16 residual /
  // accumulate keeps its loads in the store loop: 8-byte fragment accesses would waste half of every request.)
  constexpr int EPC = 16 / (int)sizeof(TC);
  constexpr int CST = BN * (int)sizeof(TC) + 16;          // 528 (bf16) / 1040 (f32) bytes per staged row
  constexpr int RPP = sizeof(TC) == 2 ? 128 : 64;         // 67.6 KB / 66.6 KB per pass
  constexpr int NPASS = BM / RPP, PPW = 128 / RPP, IPP = MI / PPW;  // passes, passes per wave row, fragment rows per pass
  constexpr int CPRo = BN / EPC;
  const TC* Rq = (const TC*)p.residual;
  auto lds_barrier = [&]() {
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();
    __builtin_amdgcn_sched_barrier(0);
  };
  {
    float bias_v[NI][4];
#pragma unroll
    for (int j = 0; j < NI; ++j)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int n = n0 + wc + j * 16 + 4 * (lane >> 4) + r;
        bias_v[j][r] = (p.bias && n < p.N) ? p.bias[n] : 0.f;
      }
#pragma unroll
    for (int i = 0; i < MI; ++i) {
      const int m = m0 + wr + i * 16 + (lane & 15);
      const float rv = (p.rowvec && m < p.M) ? p.rowvec[m] : 0.f;
#pragma unroll
      for (int j = 0; j < NI; ++j)
#pragma unroll
        for (int r = 0; r < 4; ++r) acc[i][j][r] = p.alpha * acc[i][j][r] + (rv + bias_v[j][r]);
    }
  }
  bool late_add = (Rq != nullptr) || p.accumulate;   // residual / old C still to be added in the store loop
  if constexpr (sizeof(TC) == 4) {
    if (late_add) {
      // one fragment row (NI x 16 bytes per lane) in flight ahead of the one being added
      const int nf = n0 + wc + 4 * (lane >> 4);
      auto load_row = [&](int i, f32x4 (&dst)[NI], const float* src, long ld) {
        const int m = m0 + wr + i * 16 + (lane & 15);
#pragma unroll
        for (int j = 0; j < NI; ++j)
          dst[j] = (m < p.M && (nf + j * 16) < p.N) ? *(const f32x4*)(src + (long)m * ld + nf + j * 16) : f32x4{0.f, 0.f, 0.f, 0.f};
      };
      auto add_all = [&](const float* src, long ld) {
        f32x4 rr[2][NI];
        load_row(0, rr[0], src, ld);
#pragma unroll
        for (int i = 0; i < MI; ++i) {
          if (i + 1 < MI) load_row(i + 1, rr[(i + 1) & 1], src, ld);
#pragma unroll
          for (int j = 0; j < NI; ++j) acc[i][j] += rr[i & 1][j];
        }
      };
      if (Rq) add_all((const float*)Rq, p.ldr);
      if (p.accumulate) add_all((const float*)Cp, p.ldc);
      late_add = false;
    }
  }
  // every load so far has been consumed (the compiler waited for it at its use): from here on the f32 path only stores
  // (Measured, no gain: taking each pass's rows from both wave rows so that all eight waves write LDS in every pass - the
  //  epilogue's 9.5-10.6 k cycles are the 128 KiB of stores going through the CU's vector-memory path, not the staging.)
#pragma unroll
  for (int pass = 0; pass < NPASS; ++pass) {
    lds_barrier();
    if ((wave >> 2) == pass / PPW) {
#pragma unroll
      for (int ii = 0; ii < IPP; ++ii) {
        const int i = (pass % PPW) * IPP + ii;
        const int ml = wr + i * 16 + (lane & 15);
#pragma unroll
        for (int j = 0; j < NI; ++j) {
          const int nl = wc + j * 16 + 4 * (lane >> 4);
          const float v[4] = {acc[i][j][0], acc[i][j][1], acc[i][j][2], acc[i][j][3]};
          OutVec<TC>::store4((TC*)(smem + (ml - pass * RPP) * CST) + nl, v);
        }
      }
    }
    lds_barrier();
#pragma unroll
    for (int it = 0; it < (RPP * CPRo) / NT; ++it) {
      const int c = threadIdx.x + NT * it;
      const int row = c / CPRo, col = (c % CPRo) * EPC;
      const int m = m0 + pass * RPP + row, n = n0 + col;
      if (m < p.M && n < p.N) {
        u32x4 w = *(const u32x4*)(smem + row * CST + col * (int)sizeof(TC));
        if constexpr (sizeof(TC) == 2) {
          if (late_add) {
            float o[EPC];
#pragma unroll
            for (int e = 0; e < 4; ++e) { o[2 * e] = __uint_as_float(w[e] << 16); o[2 * e + 1] = __uint_as_float(w[e] & 0xffff0000u); }
            auto add16 = [&](const TC* src) {
              const u32x4 t = *(const u32x4*)src;
#pragma unroll
              for (int e = 0; e < 4; ++e) { o[2 * e] += __uint_as_float(t[e] << 16); o[2 * e + 1] += __uint_as_float(t[e] & 0xffff0000u); }
            };
            if (Rq) add16(Rq + (long)m * p.ldr + n);
            if (p.accumulate) add16(Cp + (long)m * p.ldc + n);
#pragma unroll
            for (int e = 0; e < 4; ++e) w[e] = pack2_bf16(o[2 * e], o[2 * e + 1]);
          }
        }
        *(u32x4*)(Cp + (long)m * p.ldc + n) = w;
      }
    }
  }
  G256_TS(3)
}

// BKV = 64: two 64 KiB stages of 64-wide K-tiles (H: half operands, f32 output); 32: five 32 KiB stages of 32-wide K-tiles
template <typename TC, int AL, int BL, int BKV, bool H = false>
__global__ __launch_bounds__(512, 2) void kernel(GemmParams p) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  static_assert(!H || (BKV == 64 && sizeof(TC) == 4), "half operands: the 64-wide K loop with f32 output");
  G256_TS(0)
  const int ntm = (p.M + BM - 1) / BM, ntn = (p.N + BN - 1) / BN;
  tile_body<TC, std::conditional_t<BKV == 64, Pipe<AL, BL, H>, Pipe32<AL, BL>>>(p, xcd_tile_index(ntm * ntn), smem);
}

template <typename TC, int AL, int BL>
__global__ __launch_bounds__(512, 2) void kernel_x3(GemmParams p) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  G256_TS(0)
  const int ntm = (p.M + BM - 1) / BM, ntn = (p.N + BN - 1) / BN;
  tile_body<TC, PipeX3<AL, BL>>(p, xcd_tile_index(ntm * ntn), smem);
}

// ---- grouped launch: the tiles of up to MAXG independent products in ONE grid (the four weight gradients of a transformer layer:
// 72 + 36 + 27 + 9 tiles at config B).  Each product alone needs a deep K split to fill 256 CUs (out-proj: 9 tiles x 28 slices of 9
// K-tiles each, a third of such a block is prologue + f32 epilogue) and ends in its own ragged round; together they fill the chip with
// one or two slices of >= 128 K-tiles per tile.  blockIdx.x walks the concatenated tile lists (XCD-swizzled as a whole: neighbouring
// tiles of a product still share their operand panels in one XCD's L2), blockIdx.y is the K slice, the same for every product.
constexpr int MAXG = 8;
struct GroupParams {
  GemmParams p[MAXG];
  int tile_start[MAXG + 1];   // first global tile index of each product (tile_start[n] = total)
  int n;
};
template <typename TC, int AL, int BL, bool H = false>
__global__ __launch_bounds__(512, 2) void kernel_group(const GroupParams gp) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  const int gt = xcd_tile_index(gp.tile_start[gp.n]);
  int pi = 0;
#pragma unroll
  for (int k = 1; k < MAXG; ++k) pi += (k < gp.n && gt >= gp.tile_start[k]) ? 1 : 0;
  pi = __builtin_amdgcn_readfirstlane(pi);
  const GemmParams p = gp.p[pi];
  tile_body<TC, Pipe<AL, BL, H>>(p, gt - gp.tile_start[pi], smem);
}

}  // namespace g256
