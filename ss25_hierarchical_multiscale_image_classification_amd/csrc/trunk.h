// The op sequence of the ResNet18 trunk: stem, max-pool and the four stages, per precision.
#pragma once
#include <type_traits>
#include "conv_launch.h"
#include "stem.h"
#include "pool.h"
#include "block16_c64.h"

namespace hipac {

// The trunk is a fixed sequence of 21 launches ("ops"): 0 stem, 1 max-pool, then per
// stage conv1(b0) [proj] conv2(b0) conv1(b1) conv2(b1).  `first..last` selects a
// sub-range (whole trunk by default) so single layers can be timed / profiled.
struct OpRange {
  int first, last, next;
  bool take() {
    const int i = next++;
    return i >= first && i <= last;
  }
};

// What the stages of one trunk run share.  `l1_fused` is read by stage 0 only (the 16-bit single-value precisions), `pool_part`
// by the last stage only: not null = the network's last conv leaves the per-image partial sums of the global average pool there
// (halo16.h, POOL) instead of the fp32 map.  `qm`: precision fp16q8.
struct StageEnv {
  const Net& net;
  hipStream_t s;
  OpRange& ops;
  Q8Map qm;
  bool l1_fused;
  void* pool_part;
};

// One ResNet stage = two BasicBlocks.  CI/HI: input channels / spatial size,
// CO/HO: output.  STRIDE 2 stages carry the 1x1/2 projection shortcut.
//
// The pair modes on halo16x2.h -- PM 1: precision fp16q8 (pair + q8 tensors), PM 2: fp16x3 (pairs only, three f16 products).
// Stride-2 stages: the entry conv on the parity-plane form, the 1x1 / stride 2 projection shortcut folded into the block's second
// conv as extra K steps (its op slot is empty).  A block's first conv leaves the lo plane out in fp16q8 (nothing reads it).
template <int PM, int CI, int CO, int HI, int STRIDE, bool LAST>
static int run_stage_pairs(StageEnv& e, int stage, const void* x, void* tmp, void* o0, void* o1, int n) {
  constexpr int HO = HI / STRIDE;
  const Net& net = e.net;
  const ConvW(&bw)[2] = net.block[2 * stage];
  const ConvW(&bw1)[2] = net.block[2 * stage + 1];
  hipStream_t s = e.s;
  OpRange& ops = e.ops;
  auto Q = [&](const void* pairs) -> void* { return PM == 1 ? e.qm.of(pairs) : nullptr; };
  if constexpr (STRIDE == 1) {
    if (ops.take()) HIPAC_TRY((launch_pairconv<PM, CI, CO, HO, false, true, false, false, false, 0, false>(x, Q(x), bw[0], nullptr, tmp, Q(tmp), n, s)));
    if (ops.take()) HIPAC_TRY((launch_pairconv<PM, CO, CO, HO, true, true, false>(tmp, Q(tmp), bw[1], x, o0, Q(o0), n, s)));
  } else {
    if (ops.take()) HIPAC_TRY((launch_pairconv<PM, CI, CO, HO, false, true, false, false, true, 0, false>(x, Q(x), bw[0], nullptr, tmp, Q(tmp), n, s)));
    (void)ops.take();
    if (ops.take())
      HIPAC_TRY((launch_pairconv<PM, CO, CO, HO, false, true, false, false, false, CI>(tmp, Q(tmp), bw[1], x, o0, Q(o0), n, s, Q(x), net.down[stage - 1].w,
                                                                                        net.bias_c2p[stage - 1])));
  }
  if (ops.take()) HIPAC_TRY((launch_pairconv<PM, CO, CO, HO, false, true, false, false, false, 0, false>(o0, Q(o0), bw1[0], nullptr, tmp, Q(tmp), n, s)));
  if (ops.take()) {
    if constexpr (LAST) {
      if (e.pool_part) HIPAC_TRY((launch_pairconv<PM, CO, CO, HO, true, false, true>(tmp, Q(tmp), bw1[1], o0, e.pool_part, nullptr, n, s)));
      else HIPAC_TRY((launch_pairconv<PM, CO, CO, HO, true, false, false, true>(tmp, Q(tmp), bw1[1], o0, o1, nullptr, n, s)));
    } else {
      HIPAC_TRY((launch_pairconv<PM, CO, CO, HO, true, true, false>(tmp, Q(tmp), bw1[1], o0, o1, Q(o1), n, s)));  // (its q8 tensor feeds the next stage's entry conv)
    }
  }
  return 0;
}

// the single-value precisions (bf16, fp16, fp32)
template <typename T, int CI, int CO, int HI, int STRIDE, bool LAST>
static int run_stage_single(StageEnv& e, int stage, const void* x, void* tmp, void* ds, void* o0, void* o1, int n) {
  constexpr int HO = HI / STRIDE;
  const Net& net = e.net;
  const ConvW(&bw)[2] = net.block[2 * stage];
  const ConvW(&bw1)[2] = net.block[2 * stage + 1];
  const char* z = net.zero_page;
  hipStream_t s = e.s;
  OpRange& ops = e.ops;
  // second conv of the stage's second block; for the network's last one (LAST) either the fp32 map or, with `pool_part`,
  // the per-image partial sums of the global average pool (halo16.h, POOL; the 16-bit precisions)
  auto launch_last = [&](const void* in_, const void* resid_, void* out_) -> int {
    if constexpr (LAST && sizeof(T) == 2) {
      if (e.pool_part)
        return launch_conv<T, CO, CO, HO, HO, 3, 1, true, true, true, false, true>(in_, bw1[1], resid_, e.pool_part, n, s, z);
    }
    return launch_conv<T, CO, CO, HO, HO, 3, 1, true, true, LAST>(in_, bw1[1], resid_, out_, n, s, z);
  };
  if constexpr (CI == 64 && CO == 64 && HI == 56 && STRIDE == 1 && sizeof(T) == 2) {
    if (e.l1_fused) {
      // layer1: each BasicBlock is one launch (conv1 -> conv2 + shortcut on chip); the conv2 op slots stay empty
      const int per_xcd = 4 * ((n + 7) / 8);                   // strips on the busiest XCD
      const int grid = 8 * (per_xcd < 32 ? per_xcd : 32);      // persistent: one 8-wave workgroup per CU
      auto block = [&](const ConvW(&w)[2], const void* in, void* out) -> int {
        hipLaunchKernelGGL(block16_c64_kernel<T>, dim3(grid), dim3(512), 0, s, (const T*)in, (const T*)w[0].w, w[0].bias,
                           (const T*)w[1].w, w[1].bias, (T*)out, n);
        return (int)hipGetLastError();
      };
      if (ops.take()) HIPAC_TRY(block(bw, x, o0));
      (void)ops.take();
      if (ops.take()) HIPAC_TRY(block(bw1, o0, o1));
      (void)ops.take();
      return 0;
    }
  }
  // block 0
  const void* idt = x;
  if constexpr (STRIDE == 2 && sizeof(T) == 2) {
    if (net.projk && net.bias_c2p[stage - 1]) {
      // layers 2-4: plain 3x3/2 entry conv; the projection rides in the SECOND conv as extra K steps (its op slot is empty)
      if (ops.take())
        HIPAC_TRY((launch_conv<T, CI, CO, HI, HI, 3, STRIDE, true, false, false>(x, bw[0], nullptr, tmp, n, s, z)));
      (void)ops.take();
      if (ops.take())
        HIPAC_TRY((launch_conv_projk<T, CO, HO, CI>(tmp, bw[1], net.down[stage - 1], net.bias_c2p[stage - 1], x, o0, n, s, z)));
      if (ops.take()) HIPAC_TRY((launch_conv<T, CO, CO, HO, HO, 3, 1, true, false, false>(o0, bw1[0], nullptr, tmp, n, s, z)));
      if (ops.take()) HIPAC_TRY((launch_last(tmp, o0, o1)));
      return 0;
    }
  }
  if constexpr (STRIDE == 2 && sizeof(T) == 2 && CO <= 256) {
    // one launch: conv1 and the projection shortcut (the op slot of the projection stays empty).
    // Not for layer4: its second accumulator set pushes the kernel past 256 registers, i.e. to
    // one workgroup per CU (measured 349 ns/img fused vs 132 + 37 separate).
    if (ops.take()) HIPAC_TRY((launch_down<T, CI, CO, HI>(x, bw[0], net.down[stage - 1], tmp, ds, n, s, z)));
    (void)ops.take();
    idt = ds;
  } else {
    if (ops.take())
      HIPAC_TRY((launch_conv<T, CI, CO, HI, HI, 3, STRIDE, true, false, false>(x, bw[0], nullptr, tmp, n, s, z)));
    if constexpr (STRIDE != 1 || CI != CO) {
      if (ops.take())
        HIPAC_TRY((launch_conv<T, CI, CO, HI, HI, 1, STRIDE, false, false, false>(x, net.down[stage - 1], nullptr, ds, n, s, z)));
      idt = ds;
    }
  }
  if (ops.take()) HIPAC_TRY((launch_conv<T, CO, CO, HO, HO, 3, 1, true, true, false>(tmp, bw[1], idt, o0, n, s, z)));
  // block 1
  if (ops.take()) HIPAC_TRY((launch_conv<T, CO, CO, HO, HO, 3, 1, true, false, false>(o0, bw1[0], nullptr, tmp, n, s, z)));
  if (ops.take()) HIPAC_TRY((launch_last(tmp, o0, o1)));
  return 0;
}

template <typename T, int PM, int CI, int CO, int HI, int STRIDE, bool LAST = false>  // PM: pair mode (0: single values)
static int run_stage(StageEnv& e, int stage, const void* x, void* tmp, void* ds, void* o0, void* o1, int n) {
  if constexpr (PM != 0) {
    static_assert(sizeof(T) == 2, "the pair layout");
    return run_stage_pairs<PM, CI, CO, HI, STRIDE, LAST>(e, stage, x, tmp, o0, o1, n);
  } else {
    return run_stage_single<T, CI, CO, HI, STRIDE, LAST>(e, stage, x, tmp, ds, o0, o1, n);
  }
}

// Ops 0 (stem) and 1 (max-pool): xin -> the pooled map at p.pool (pair modes: (hi, lo) pairs, fp16q8 also its q8 tensor).
//
//   precision           u8_input && stem_strip   fuse_stem   form
//   fp16x3, fp16q8      yes                      any         strip kernel (SPLIT; Q8 in fp16q8), op 1 empty
//   fp16x3, fp16q8      no                       any         unfused: exact f32 stem (fp32 NHWC4 input) + pair-writing pool
//   bf16, fp16          yes                      1           strip kernel, op 1 empty
//   bf16, fp16          no                       1           fused tile kernel (uint8 or NHWC4 input), op 1 empty
//   bf16, fp16          any                      0           unfused: stem conv + max-pool in T
//   fp32                any                      any         unfused: stem conv + max-pool in T
template <typename T, int PM>
static int run_stem(const Net& net, const Plan& p, char* ws, const void* xin, int ne, hipStream_t s, OpRange& ops, const Q8Map& qm) {
  constexpr bool PAIRS = PM != 0;
  T* const pool = (T*)(ws + p.pool);
  if constexpr (sizeof(T) == 2) {
    if (p.u8_input && p.stem_strip && (PAIRS || p.fuse_stem)) {
      // pair modes: split weights (the bytes are exact in fp16)
      if (ops.take()) {
        const int n_strips = 2 * ne;
        const int n_pairs = (n_strips + 1) / 2;
        const int sgrid = n_pairs < 256 ? n_pairs : 256;  // persistent: one 8-wave workgroup (two teams) per CU
        hipLaunchKernelGGL((stem_pool_strip2_kernel<T, PAIRS, PM == 1>), dim3(sgrid), dim3(512), 0, s, (const unsigned char*)xin,
                           (const T*)net.stem_u8.w, net.stem_u8.bias, pool, n_strips, ne * kPatch * kPatch * 3,
                           PM == 1 ? (unsigned char*)qm.of(pool) : nullptr);
        HIPAC_TRY((int)hipGetLastError());
      }
      (void)ops.take();
      return 0;
    }
    if constexpr (!PAIRS) {
      if (p.fuse_stem) {
        // the 112x112 stem map is never materialised
        if (ops.take()) {
          const int n_tiles = ne * kStemTilesPerImage;
          const int grid = n_tiles < 512 ? n_tiles : 512;  // persistent: 2 workgroups per CU
          if (p.u8_input)
            hipLaunchKernelGGL((stem_pool_kernel<T, true>), dim3(grid), dim3(256), 0, s, xin, (const T*)net.stem.w, net.stem.bias, pool,
                               n_tiles, net.lut_t, (long long)ne * kPatch * kPatch * 3);
          else
            hipLaunchKernelGGL((stem_pool_kernel<T, false>), dim3(grid), dim3(256), 0, s, xin, (const T*)net.stem.w, net.stem.bias, pool,
                               n_tiles, (const unsigned short*)nullptr, 0LL);
          HIPAC_TRY((int)hipGetLastError());
        }
        (void)ops.take();
        return 0;
      }
    }
  }
  using TS = std::conditional_t<PAIRS, float, T>;  // element type of the input and of the stem map
  if (ops.take())
    HIPAC_TRY((launch_conv<TS, 4, 64, 224, 224, 7, 2, true, false, false, true>(xin, net.stem, nullptr, ws + p.stem, ne, s)));
  if (ops.take()) {
    const long long total = (long long)ne * 56 * 56 * 8;
    const dim3 grid((unsigned)((total + 255) / 256));
    if constexpr (PAIRS) hipLaunchKernelGGL((maxpool3x3s2_split_kernel<_Float16>), grid, dim3(256), 0, s, (const float*)(ws + p.stem), pool, ne);
    else hipLaunchKernelGGL((maxpool3x3s2_kernel<T>), grid, dim3(256), 0, s, (const T*)(ws + p.stem), pool, ne);
    HIPAC_TRY((int)hipGetLastError());
    if constexpr (PM == 1) HIPAC_TRY(launch_pairs_to_q8(pool, qm.of(pool), (long long)ne * 56 * 56, 64, s));
  }
  return 0;
}

template <typename T, int PM = 0>  // PM: pair mode (run_stage)
static int run_trunk(const Net& net, const Plan& p, char* ws, const void* xin, int n_early, int img_off, int n_late,
                     hipStream_t s, int first, int last) {
  OpRange ops{first, last, 0};
  const int ne = n_early, nl = n_late;
  StageEnv e{net, s, ops, Q8Map{ws, p.q8}, p.l1_fused != 0, p.pool_head && sizeof(T) == 2 ? ws + p.part : nullptr};
  HIPAC_TRY((run_stem<T, PM>(net, p, ws, xin, ne, s, ops, e.qm)));
  // layer2's second block writes straight into this sub-batch's slice of the group buffer
  char* l2out = ws + p.blk[3] + (size_t)img_off * 28 * 28 * 128 * p.esz;
  HIPAC_TRY((run_stage<T, PM, 64, 64, 56, 1>(e, 0, ws + p.pool, ws + p.tmp_e, nullptr, ws + p.blk[0], ws + p.blk[1], ne)));
  HIPAC_TRY((run_stage<T, PM, 64, 128, 56, 2>(e, 1, ws + p.blk[1], ws + p.tmp_e, ws + p.ds_e, ws + p.blk[2], l2out, ne)));
  HIPAC_TRY((run_stage<T, PM, 128, 256, 28, 2>(e, 2, ws + p.blk[3], ws + p.tmp_l, ws + p.ds_l, ws + p.blk[4], ws + p.blk[5], nl)));
  HIPAC_TRY((run_stage<T, PM, 256, 512, 14, 2, true>(e, 3, ws + p.blk[5], ws + p.tmp_l, ws + p.ds_l, ws + p.blk[6], ws + p.blk[7], nl)));
  return 0;
}

}  // namespace hipac
