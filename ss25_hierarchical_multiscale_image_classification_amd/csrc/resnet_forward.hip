// The ResNet18 forward driver of the C ABI: workspace plan, the split of a batch into sub-batches, groups and
// launch lanes, and the entry points that run the trunk (forward, run_ops, tap).
#include "resnet_handle.h"
#include "../../include/hipac_pair_tap.h"

namespace hipac {

Plan make_plan(int batch, int precision) {
  Plan p;
  p.esz = elem_size(precision);
  // bc: early sub-batch -- 512 images give layer1/2 thousands of tiles (block-round
  // quantisation < 10 %).  gc: late group -- layer4 has only 49 pixels per image, so it
  // needs thousands of images (default group 4096) to fill 256 CUs x 2 workgroups for several rounds.
  // (tuning knobs; a whole run must use one setting)
  const int bc_cap = env_int("HIPAC_SUBBATCH", 512, 1, 1024);
  int gc_cap = env_int("HIPAC_GROUP", 4096, 1, 8192);
  // fp16q8: halo16x2.h addresses its pair tensors with 32-bit byte offsets (buffer descriptors): layer3's stride-2 entry conv sees
  // 4 x gc x 196 pixels x 128 channels x 4 bytes, which stays below 2^31 up to gc = 5 349
  if (pair_mode(precision) && gc_cap > 4096) gc_cap = 4096;
  p.fuse_stem = wide_mode(precision) ? 0 : env_int("HIPAC_FUSE_STEM", 1, 0, 1);
  p.u8_input = 0;
  p.stem_strip = env_int("HIPAC_STEM_STRIP", 1, 0, 1);
  p.l1_fused = wide_mode(precision) ? 0 : env_int("HIPAC_L1_FUSED", 1, 0, 1);
  p.pool_head = precision == HIPAC_PREC_FP32 ? 0 : env_int("HIPAC_POOL_HEAD", 1, 0, 1);
  if (batch < 1) batch = 1;
  p.bc = batch < bc_cap ? batch : bc_cap;
  p.gc = batch < gc_cap ? batch : gc_cap;
  if (p.gc < p.bc) p.gc = p.bc;
  p.gc = (p.gc + p.bc - 1) / p.bc * p.bc;  // whole sub-batches per group
  const size_t b = (size_t)p.bc, g = (size_t)p.gc;
  size_t off = 0;
  auto take = [&](size_t bytes) {
    size_t o = off;
    off += align256(bytes);
    return o;
  };
  const size_t e = (size_t)p.esz;
  p.xin = take(b * kPadH * kPadW * 4 * e);
  p.stem = take(b * 112 * 112 * 64 * e);
  p.pool = take(b * 56 * 56 * 64 * e);
  p.tmp_e = take(b * 56 * 56 * 64 * e);
  p.ds_e = take(b * 28 * 28 * 128 * e);
  p.blk[0] = take(b * 56 * 56 * 64 * e);
  p.blk[1] = take(b * 56 * 56 * 64 * e);
  p.blk[2] = take(b * 28 * 28 * 128 * e);
  p.blk[3] = take(g * 28 * 28 * 128 * e);
  p.tmp_l = take(g * 14 * 14 * 256 * e);
  p.ds_l = take(g * 14 * 14 * 256 * e);
  p.blk[4] = take(g * 14 * 14 * 256 * e);
  p.blk[5] = take(g * 14 * 14 * 256 * e);
  p.blk[6] = take(g * 7 * 7 * 512 * e);
  p.blk[7] = take(g * 7 * 7 * 512 * 4);
  p.part = take(((g * 49 + 255) / 256) * 2 * 7 * 2 * 512 * 4);
  p.q8 = 0;
  if (precision == HIPAC_PREC_FP16Q8) {
    const size_t pairs_end = p.blk[7];  // every pair tensor lies below the fp32 map
    p.q8 = take(pairs_end / 2 + 256);
  }
  p.total = off;
  return p;
}

// Split of one forward call into lanes.  Each lane owns a whole workspace plan.
struct Lanes {
  int n;        // 1 .. kMaxLanes
  int chunk;    // images handled by every lane but the last (which takes the rest)
  Plan p;       // per-lane plan (sized for `chunk` images)
  size_t total; // workspace bytes
};
static Lanes make_lanes(int batch, int precision) {
  Lanes L;
  const Plan single = make_plan(batch, precision);
  int want = env_int("HIPAC_LANES", 2, 1, kMaxLanes);
  while (want > 1 && batch < 2 * want * single.bc) --want;  // every lane gets at least two sub-batches
  L.n = want;
  if (L.n == 1) {
    L.chunk = batch, L.p = single, L.total = single.total;
    return L;
  }
  L.chunk = ((batch + L.n - 1) / L.n + single.bc - 1) / single.bc * single.bc;  // whole sub-batches per lane
  while (L.n > 1 && (long long)(L.n - 1) * L.chunk >= batch) --L.n;                  // (rounding up may empty the last lanes)
  L.p = make_plan(L.chunk, precision);
  // run_ops / tap address the workspace with the single-lane plan of `batch`: keep room for it
  L.total = (size_t)L.n * L.p.total > single.total ? (size_t)L.n * L.p.total : single.total;
  return L;
}

using TrunkFn = int (*)(const Net&, const Plan&, char*, const void*, int, int, int, hipStream_t, int, int);
static TrunkFn trunk_for(int precision) {
  switch (precision) {
    case HIPAC_PREC_BF16: return run_trunk_bf16;
    case HIPAC_PREC_FP16: return run_trunk_f16;
    case HIPAC_PREC_FP16X3: return run_trunk_f16x3;
    case HIPAC_PREC_FP16Q8: return run_trunk_f16q8;
    default: return run_trunk_f32;  // a handle holds one of the five: hipac_resnet18_pack refuses any other
  }
}

// Applies the caller's input layout to the plan: sets u8_input (the stem kernel reads the raw uint8 patches) and returns
// whether the stem instead reads p.xin of the workspace, i.e. the input has to be converted into it first.
// By run_stem's table (trunk.h) a stem form that takes bytes exists in the pair modes with the strip kernel
// (stem_strip) and in bf16 / fp16 with the fused stem (fuse_stem: strip or tile kernel); fp32 has none (its fuse_stem
// is 0).  Only the pair modes have a uint8 conversion (launch_u8_to_nhwc4_f32): forward refuses the other cases.
static bool apply_input_layout(Plan& p, int precision, int in_layout) {
  const bool stem_takes_u8 = pair_mode(precision) ? p.stem_strip : p.fuse_stem;
  p.u8_input = in_layout == HIPAC_IN_U8_HWC && stem_takes_u8;
  return in_layout == HIPAC_IN_NCHW_F32 || (in_layout == HIPAC_IN_U8_HWC && !p.u8_input);
}

// include/hipac_pair_tap.h: where (map, plane) lies in the workspace of plan p, and how many bytes `batch` images of it are.
// false for a combination the header refuses.
struct PairTapSpan {
  size_t off, bytes;
};
static bool pair_tap_span(const Plan& p, int precision, int batch, int map, int plane, PairTapSpan* out) {
  if (batch < 1 || !pair_mode(precision)) return false;
  if (map < HIPAC_PAIR_TAP_POOL || map > HIPAC_PAIR_TAP_INNER0 + 7) return false;
  if (plane != HIPAC_PAIR_TAP_PLANE_PAIRS && plane != HIPAC_PAIR_TAP_PLANE_Q8) return false;
  const bool last = map == HIPAC_PAIR_TAP_BLOCK0 + 7;
  if (plane == HIPAC_PAIR_TAP_PLANE_Q8 && (precision != HIPAC_PREC_FP16Q8 || last)) return false;
  const int ch[4] = {64, 128, 256, 512}, hw[4] = {56, 28, 14, 7};
  size_t pairs;  // offset of the pair tensor (map 9: of the fp32 map)
  int st = 0;
  if (map == HIPAC_PAIR_TAP_POOL) {
    pairs = p.pool;
  } else if (map < HIPAC_PAIR_TAP_INNER0) {
    st = (map - HIPAC_PAIR_TAP_BLOCK0) / 2;
    pairs = p.blk[map - HIPAC_PAIR_TAP_BLOCK0];
  } else {
    st = (map - HIPAC_PAIR_TAP_INNER0) / 2;
    pairs = st < 2 ? p.tmp_e : p.tmp_l;
  }
  const size_t elems = (size_t)batch * hw[st] * hw[st] * ch[st];
  if (plane == HIPAC_PAIR_TAP_PLANE_Q8) *out = {p.q8 + pairs / 2, elems * 2};  // Q8Map::of (conv_launch.h)
  else *out = {pairs, elems * 4};                                             // a pair or one float per element
  return true;
}

}  // namespace hipac

using namespace hipac;

extern "C" {

size_t hipac_resnet18_workspace_bytes(int batch, int precision) {
  if (batch <= 0) return 0;
  return make_lanes(batch, precision).total;
}

int hipac_resnet18_forward(const hipac_weights_t* w, const void* x, int batch, int in_layout, float* feats,
                           float* logits, int64_t* labels, void* workspace, size_t workspace_bytes, void* stream) {
  HIPAC_REQUIRE(w && x && workspace, HIPAC_EINVAL, "forward: null argument");
  HIPAC_REQUIRE(batch > 0, HIPAC_EINVAL, "forward: batch %d", batch);
  HIPAC_REQUIRE(in_layout == HIPAC_IN_NCHW_F32 || in_layout == HIPAC_IN_NHWC4_PAD || in_layout == HIPAC_IN_U8_HWC,
                HIPAC_EINVAL, "forward: unknown in_layout %d", in_layout);
  HIPAC_REQUIRE(!(logits || labels) || w->net.num_classes > 0, HIPAC_EINVAL,
                "forward: logits/labels requested but the weights carry no fc (fc = Identity)");
  HIPAC_REQUIRE(((uintptr_t)workspace & 255) == 0, HIPAC_EINVAL, "forward: workspace must be 256-byte aligned");
  HIPAC_REQUIRE(((uintptr_t)x & 15) == 0, HIPAC_EINVAL, "forward: x must be 16-byte aligned");
  {
    int dev = -1;
    HIPAC_CHECK_HIP(hipGetDevice(&dev));
    HIPAC_REQUIRE(dev == w->device, HIPAC_EINVAL, "forward: handle was packed on device %d, current device is %d",
                  w->device, dev);
  }
  const Net& net = w->net;
  const Lanes L = make_lanes(batch, net.precision);
  Plan p = L.p;
  HIPAC_REQUIRE(workspace_bytes >= L.total, HIPAC_EWORKSPACE, "forward: workspace %zu < required %zu",
                workspace_bytes, L.total);
  HIPAC_REQUIRE(in_layout != HIPAC_IN_U8_HWC || p.fuse_stem || pair_mode(net.precision), HIPAC_EUNSUPPORTED,
                "forward: uint8 input needs the fused stem (bf16 / fp16 weights, HIPAC_FUSE_STEM not 0) or fp16x3");
  const bool convert = apply_input_layout(p, net.precision, in_layout);  // (uint8: a pair mode without the strip kernel)
  // an input the stem reads in place: raw patches (normalise fused in the stem) or the native layout
  const size_t in_img_bytes = p.u8_input ? (size_t)kPatch * kPatch * 3 : (size_t)kPadH * kPadW * 4 * p.esz;
  const TrunkFn trunk = trunk_for(net.precision);
  // images [i0, i0 + n) on stream s with the lane's own workspace
  auto run_lane = [&](char* ws, int i0, int n, hipStream_t s) -> int {
    for (int g0 = i0; g0 < i0 + n; g0 += p.gc) {
      const int gn = i0 + n - g0 < p.gc ? i0 + n - g0 : p.gc;
      for (int b0 = 0; b0 < gn; b0 += p.bc) {
        const int bn = gn - b0 < p.bc ? gn - b0 : p.bc;
        const void* xin = ws + p.xin;
        if (!convert) {
          xin = (const char*)x + (size_t)(g0 + b0) * in_img_bytes;  // the stem reads the caller's buffer
        } else {
          int rc = in_layout == HIPAC_IN_NCHW_F32
                       ? launch_nchw_to_nhwc4((const float*)x + (size_t)(g0 + b0) * 3 * kPatch * kPatch, ws + p.xin, bn,
                                              net.precision, s)
                       : launch_u8_to_nhwc4_f32((const unsigned char*)x + (size_t)(g0 + b0) * kPatch * kPatch * 3,
                                                net.lut_f32, (float*)(ws + p.xin), bn, s);
          HIPAC_REQUIRE(rc == 0, rc, "forward: input conversion launch failed (%d)", rc);
        }
        int rc = trunk(net, p, ws, xin, bn, b0, 0, s, 0, kNumEarlyOps - 1);
        if (rc) return rc;
      }
      int rc = trunk(net, p, ws, nullptr, 0, 0, gn, s, kNumEarlyOps, kNumOps - 1);
      if (rc) return rc;
      float* const f = feats ? feats + (size_t)g0 * 512 : nullptr;
      float* const lg = logits ? logits + (size_t)g0 * net.num_classes : nullptr;
      int64_t* const lb = labels ? labels + g0 : nullptr;
      rc = p.pool_head ? launch_head_pool((const float*)(ws + p.part), gn, net.fc_w, net.fc_b, net.num_classes, f, lg, lb, s)
                       : launch_head((const float*)(ws + p.blk[7]), gn, net.fc_w, net.fc_b, net.num_classes, f, lg, lb, s);
      HIPAC_REQUIRE(rc == 0, rc, "forward: head launch failed (%d)", rc);
    }
    return 0;
  };
  hipStream_t s = (hipStream_t)stream;
  char* ws = (char*)workspace;
  auto lane_s = [&](int k) { return k == 0 ? s : w->lane_stream[k - 1]; };
  int n_lanes = L.n;
  for (int k = 1; k < n_lanes; ++k)
    if (!lane_s(k)) n_lanes = 1;  // a stream could not be created at pack time: single lane
  if (n_lanes == 1) {
    if (L.n == 1) return run_lane(ws, 0, batch, s);
    // the plan `p` is sized for one lane's chunk: walk the chunks one after another on the caller's stream
    for (int i0 = 0; i0 < batch; i0 += L.chunk) {
      int rc1 = run_lane(ws, i0, batch - i0 < L.chunk ? batch - i0 : L.chunk, s);
      if (rc1) return rc1;
    }
    return 0;
  }
  // fork: lanes 1.. (the handle's streams) start after everything already queued on s; join: s waits for all of them
  hipEvent_t fork = nullptr, join[kMaxLanes] = {nullptr, nullptr, nullptr, nullptr};
  HIPAC_CHECK_HIP(hipEventCreateWithFlags(&fork, hipEventDisableTiming));
  hipError_t e = hipSuccess;
  for (int k = 1; k < n_lanes && e == hipSuccess; ++k) e = hipEventCreateWithFlags(&join[k], hipEventDisableTiming);
  int rc = 0;
  if (e == hipSuccess) e = hipEventRecord(fork, s);
  if (e == hipSuccess) {
    for (int k = n_lanes - 1; k >= 1 && e == hipSuccess; --k) {
      e = hipStreamWaitEvent(lane_s(k), fork, 0);
      if (e != hipSuccess) break;
      const int i0 = k * L.chunk, n = batch - i0 < L.chunk ? batch - i0 : L.chunk;
      if (rc == 0) rc = run_lane(ws + (size_t)k * L.p.total, i0, n, lane_s(k));
      // join even after a failed launch so the caller's stream stays ordered behind every lane
      e = hipEventRecord(join[k], lane_s(k));
    }
    if (rc == 0 && e == hipSuccess) rc = run_lane(ws, 0, L.chunk, s);
    for (int k = 1; k < n_lanes; ++k)
      if (join[k] && e == hipSuccess) e = hipStreamWaitEvent(s, join[k], 0);
  }
  (void)hipEventDestroy(fork);  // released by the runtime once the recorded work has completed
  for (int k = 1; k < n_lanes; ++k)
    if (join[k]) (void)hipEventDestroy(join[k]);
  HIPAC_CHECK_HIP(e);
  return rc;
}

int hipac_resnet18_run_ops(const hipac_weights_t* w, const void* x, int in_layout, void* workspace,
                           size_t workspace_bytes, int batch, int first_op, int last_op, void* stream) {
  HIPAC_REQUIRE(w && workspace, HIPAC_EINVAL, "run_ops: null argument");
  Plan p = make_plan(batch, w->net.precision);
  HIPAC_REQUIRE(batch > 0 && batch <= p.gc, HIPAC_EINVAL, "run_ops: batch %d exceeds one group (%d)", batch, p.gc);
  HIPAC_REQUIRE(workspace_bytes >= p.total, HIPAC_EWORKSPACE, "run_ops: workspace %zu < required %zu",
                workspace_bytes, p.total);
  HIPAC_REQUIRE(first_op >= 0 && first_op <= last_op && last_op < kNumOps, HIPAC_EINVAL, "run_ops: range %d..%d",
                first_op, last_op);
  HIPAC_REQUIRE(in_layout == HIPAC_IN_NHWC4_PAD || in_layout == HIPAC_IN_U8_HWC || in_layout == HIPAC_IN_NCHW_F32,
                HIPAC_EINVAL, "run_ops: in_layout %d", in_layout);
  HIPAC_REQUIRE(first_op > 0 || x != nullptr || in_layout == HIPAC_IN_NCHW_F32, HIPAC_EINVAL,
                "run_ops: op 0 needs the input batch");
  char* ws = (char*)workspace;
  // early ops act on the first sub-batch, late ops on the whole group; an input that needs converting was
  // converted into the workspace by the preceding forward
  const void* xin = apply_input_layout(p, w->net.precision, in_layout) ? (const void*)(ws + p.xin) : x;
  const int ne = batch < p.bc ? batch : p.bc;
  return trunk_for(w->net.precision)(w->net, p, ws, xin, ne, 0, batch, (hipStream_t)stream, first_op, last_op);
}

int hipac_resnet18_tap(const hipac_weights_t* w, const void* workspace, int batch, int tap, float* dst,
                       void* stream) {
  HIPAC_REQUIRE(w && workspace && dst, HIPAC_EINVAL, "tap: null argument");
  const Plan p = make_plan(batch, w->net.precision);
  HIPAC_REQUIRE(batch > 0 && batch <= p.bc, HIPAC_EINVAL, "tap: batch %d exceeds one sub-batch (%d)", batch, p.bc);
  HIPAC_REQUIRE(tap >= 0 && tap <= 9, HIPAC_EINVAL, "tap: index %d", tap);
  const char* ws = (const char*)workspace;
  const void* src;
  int C, H, is_f32 = 0;
  if (tap == 0) {
    HIPAC_REQUIRE(!p.fuse_stem, HIPAC_EUNSUPPORTED,
                  "tap 0 (stem) does not exist when the stem is fused with the max-pool; set HIPAC_FUSE_STEM=0");
    src = ws + p.stem, C = 64, H = 112;
    is_f32 = pair_mode(w->net.precision);  // its stem map is fp32
  } else if (tap == 1) {
    src = ws + p.pool, C = 64, H = 56;
  } else {
    const int blk = tap - 2, st = blk / 2;
    const int ch[4] = {64, 128, 256, 512}, hw[4] = {56, 28, 14, 7};
    src = ws + p.blk[blk], C = ch[st], H = hw[st];
    is_f32 = blk == 7;
    if (blk == 7 && p.pool_head) {
      // the forward left the pooled partial sums, not the map: the last conv runs once more with its fp32-map epilogue
      // (same accumulators) on the activations still in the workspace
      Plan q = p;
      q.pool_head = 0;
      int rc_t = trunk_for(w->net.precision)(w->net, q, (char*)workspace, nullptr, 0, 0, batch, (hipStream_t)stream,
                                             kNumOps - 1, kNumOps - 1);
      HIPAC_REQUIRE(rc_t == 0, rc_t, "tap: re-running the last conv failed (%d)", rc_t);
    }
  }
  int rc = launch_tap_export(src, is_f32, w->net.precision, batch, C, H, H, dst, (hipStream_t)stream);
  HIPAC_REQUIRE(rc == 0, rc, "tap: launch failed (%d)", rc);
  return 0;
}

int hipac_pair_tap_abi_version(void) { return HIPAC_PAIR_TAP_ABI_VERSION; }

size_t hipac_pair_tap_bytes(int batch, int precision, int map, int plane) {
  PairTapSpan sp;
  if (batch < 1 || !pair_mode(precision)) return 0;
  return pair_tap_span(make_plan(batch, precision), precision, batch, map, plane, &sp) ? sp.bytes : 0;
}

int hipac_pair_tap_copy(const hipac_weights_t* w, void* workspace, int batch, int map, int plane, void* dst,
                        size_t dst_bytes, void* stream) {
  HIPAC_REQUIRE(w && workspace && dst, HIPAC_EINVAL, "pair_tap: null argument");
  const int precision = w->net.precision;
  HIPAC_REQUIRE(pair_mode(precision), HIPAC_EUNSUPPORTED, "pair_tap: the handle is no pair mode (fp16x3, fp16q8)");
  HIPAC_REQUIRE(batch > 0, HIPAC_EINVAL, "pair_tap: batch %d", batch);
  const Plan p = make_plan(batch, precision);
  HIPAC_REQUIRE(batch <= p.bc, HIPAC_EINVAL, "pair_tap: batch %d exceeds one sub-batch (%d)", batch, p.bc);
  PairTapSpan sp;
  HIPAC_REQUIRE(pair_tap_span(p, precision, batch, map, plane, &sp), HIPAC_EINVAL, "pair_tap: map %d, plane %d", map, plane);
  HIPAC_REQUIRE(dst_bytes == sp.bytes, HIPAC_EINVAL, "pair_tap: dst holds %zu bytes, the plane has %zu", dst_bytes, sp.bytes);
  HIPAC_REQUIRE(sp.off + sp.bytes <= p.total, HIPAC_EINVAL, "pair_tap: the plane lies outside the workspace plan");
  if (map == HIPAC_PAIR_TAP_BLOCK0 + 7 && p.pool_head) {
    // the forward left the pooled partial sums, not the map: the last conv once more with its fp32-map epilogue (as tap 9)
    Plan q = p;
    q.pool_head = 0;
    int rc_t = trunk_for(precision)(w->net, q, (char*)workspace, nullptr, 0, 0, batch, (hipStream_t)stream, kNumOps - 1, kNumOps - 1);
    HIPAC_REQUIRE(rc_t == 0, rc_t, "pair_tap: re-running the last conv failed (%d)", rc_t);
  }
  HIPAC_CHECK_HIP(hipMemcpyAsync(dst, (const char*)workspace + sp.off, sp.bytes, hipMemcpyDeviceToDevice, (hipStream_t)stream));
  return 0;
}

}  // extern "C"
