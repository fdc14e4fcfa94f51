// The weights handle of the ResNet18 C ABI and the precision predicates, shared by resnet_pack.hip (which makes
// and frees the handle), resnet_forward.hip (which runs it) and resnet_head.hip.
#pragma once
#include <stdlib.h>

#include "common.h"

namespace hipac {

static inline bool pair_mode(int precision) { return precision == HIPAC_PREC_FP16X3 || precision == HIPAC_PREC_FP16Q8; }  // (hi, lo) fp16 pairs
static inline bool wide_mode(int precision) { return precision == HIPAC_PREC_FP32 || pair_mode(precision); }
static inline int elem_size(int precision) { return wide_mode(precision) ? 4 : 2; }

static inline int env_int(const char* name, int dflt, int lo, int hi) {
  if (const char* e = getenv(name)) {
    const int v = atoi(e);
    if (v >= lo && v <= hi) return v;
  }
  return dflt;
}

constexpr int kMaxLanes = 4;

}  // namespace hipac

struct hipac_weights {
  hipac::Net net;
  // Launch lanes 1 .. kMaxLanes - 1 of hipac_resnet18_forward (created at pack time, never blocking; lane 0 is the
  // caller's stream): large batches are split into chunks that run concurrently, so the tail of every launch (partly
  // filled last round of workgroups) is covered by the other lanes' kernels.  Fork / join with the caller's stream by
  // events.  HIPAC_LANES (default 2) says how many are used; a null entry means the stream could not be created.
  hipStream_t lane_stream[hipac::kMaxLanes - 1] = {};
  int device = 0;  // the device that was current at pack time: weights, lane streams and kernel attributes live there
};
