// Host-side weight packing of the ResNet18 C ABI (BN fold + repack into the kernels' layouts) and the lifetime of
// the weights handle.
#include <math.h>
#include <string.h>

#include <vector>

#include "e4m3.h"
#include "resnet_handle.h"

namespace hipac {

// ---- host-side rounding to the storage type (round-to-nearest-even) ----------------
static inline uint16_t f32_to_bf16_bits(float f) {
  uint32_t u;
  memcpy(&u, &f, 4);
  if ((u & 0x7fffffffu) > 0x7f800000u) return (uint16_t)((u >> 16) | 0x40);  // NaN stays NaN
  u += 0x7fffu + ((u >> 16) & 1u);
  return (uint16_t)(u >> 16);
}
static inline uint16_t f32_to_f16_bits(float f) {
  _Float16 h = (_Float16)f;  // host compiler: IEEE RNE conversion
  uint16_t b;
  memcpy(&b, &h, 2);
  return b;
}
static inline float f16_bits_to_f32(uint16_t b) {
  _Float16 h;
  memcpy(&h, &b, 2);
  return (float)h;
}
static inline uint16_t to_bits(float f, int precision) {
  return precision == HIPAC_PREC_BF16 ? f32_to_bf16_bits(f) : f32_to_f16_bits(f);
}
static float round_to(float v, int precision) {
  const uint16_t b = to_bits(v, precision);
  if (precision == HIPAC_PREC_BF16) {
    const uint32_t u = (uint32_t)b << 16;
    float f;
    memcpy(&f, &u, 4);
    return f;
  }
  return f16_bits_to_f32(b);
}

// Inference BN of output channel o as y = scale * conv + bias, in double; every caller rounds in its own way.
struct BnFold {
  double scale, bias;
};
static inline BnFold bn_fold(const hipac_convbn_t& c, int o, float eps) {
  const double scale = (double)c.bn_gamma[o] / sqrt((double)c.bn_var[o] + (double)eps);
  return {scale, (double)c.bn_beta[o] - (double)c.bn_mean[o] * scale};
}

static int upload(const void* host, size_t bytes, void** dev) {
  HIPAC_CHECK_HIP(hipMalloc(dev, bytes));
  HIPAC_CHECK_HIP(hipMemcpy(*dev, host, bytes, hipMemcpyHostToDevice));
  return 0;
}
static int upload_convw(const void* w, size_t w_bytes, const std::vector<float>& bias, ConvW* out) {
  out->wscale = out->winv = 1.f;
  const int rc = upload(w, w_bytes, &out->w);
  return rc ? rc : upload(bias.data(), bias.size() * 4, (void**)&out->bias);
}

// Fold BN and repack one conv: src [Cout][Cin][ks][ks] -> dst [Cout][ks][ks][Cin].
static int pack_conv(const hipac_convbn_t& c, int cout, int cin, int ks, float eps, int precision, bool stem,
                     ConvW* out) {
  HIPAC_REQUIRE(c.conv_w && c.bn_gamma && c.bn_beta && c.bn_mean && c.bn_var, HIPAC_EINVAL,
                "pack: null tensor pointer (cout=%d cin=%d ks=%d)", cout, cin, ks);
  const int K = stem ? 7 * 32 : ks * ks * cin;
  const bool f32 = precision == HIPAC_PREC_FP32;
  std::vector<uint16_t> w(f32 ? 0 : (size_t)cout * K, 0);
  std::vector<float> w32(f32 ? (size_t)cout * K : 0, 0.f);
  std::vector<float> bias(cout);
  for (int o = 0; o < cout; ++o) {
    const BnFold bn = bn_fold(c, o, eps);
    bias[o] = (float)bn.bias;
    for (int i = 0; i < cin; ++i)
      for (int kh = 0; kh < ks; ++kh)
        for (int kw = 0; kw < ks; ++kw) {
          const float v = (float)((double)c.conv_w[(((size_t)o * cin + i) * ks + kh) * ks + kw] * bn.scale);
          const size_t k = stem ? (size_t)kh * 32 + kw * 4 + i : ((size_t)kh * ks + kw) * cin + i;
          if (f32) w32[(size_t)o * K + k] = v;
          else w[(size_t)o * K + k] = to_bits(v, precision);
        }
  }
  return f32 ? upload_convw(w32.data(), w32.size() * 4, bias, out) : upload_convw(w.data(), w.size() * 2, bias, out);
}

// The pair modes' convs (halo16x2.h; taps = 9: 3x3, taps = 1: projection): BN folded, every weight split into the fp16 pair
// (hi, lo); per output channel and tap, per 64-channel chunk 256 bytes:
//   q8 (fp16q8):      [hi: 64 fp16 | e4m3(hi * 2^-5): 64 | e4m3(lo * 2^6): 64]
//   !q8 (fp16x3):     [hi: 64 fp16 | lo: 64 fp16]
// (hi, lo) is the pair of w * 2^S (exact), S = pair_shift of the conv -- as pack_stem_u8 does it and for its reason: unscaled,
// lo ~ 2^-11 w is an fp16 subnormal for every |w| < 0.125 and carries the fewer bits the smaller the weight is, and the e4m3 rows
// have one fixed window.  The kernel's epilogue multiplies the accumulator by 2^-S (ConvW::winv; halo16x2.h).
static double folded_absmax(const hipac_convbn_t& c, int cout, int cin, int taps, float eps) {
  if (!(c.conv_w && c.bn_gamma && c.bn_beta && c.bn_mean && c.bn_var)) return 0.0;  // (pack_conv_pairs reports it)
  double wmax = 0.0;
  for (int o = 0; o < cout; ++o) {
    const double scale = bn_fold(c, o, eps).scale;
    for (size_t k = 0; k < (size_t)cin * taps; ++k) wmax = fmax(wmax, fabs((double)c.conv_w[(size_t)o * cin * taps + k] * scale));
  }
  return wmax;
}
// S = floor(log2(2^13 / max |w|)), clamped to [0, kPairShiftMax]: the largest scaled weight in [2^12, 2^13]
static int pair_shift(double wmax) {
  if (!(wmax > 0.0) || !(wmax < HUGE_VAL)) return 0;
  const int S = (int)floor(log2(8192.0 / wmax));
  return S < 0 ? 0 : (S > kPairShiftMax ? kPairShiftMax : S);
}
static int pack_conv_pairs(const hipac_convbn_t& c, int cout, int cin, int taps, float eps, bool q8, int S, ConvW* out) {
  HIPAC_REQUIRE(c.conv_w && c.bn_gamma && c.bn_beta && c.bn_mean && c.bn_var, HIPAC_EINVAL,
                "pack: null tensor pointer (cout=%d cin=%d q8)", cout, cin);
  HIPAC_REQUIRE(cin % 64 == 0, HIPAC_EINVAL, "pack: q8 layout needs cin %% 64 == 0 (%d)", cin);
  const size_t KROW = (size_t)taps * (cin / 64) * 256;
  std::vector<uint8_t> w((size_t)cout * KROW, 0);
  std::vector<float> bias(cout);
  for (int o = 0; o < cout; ++o) {
    const BnFold bn = bn_fold(c, o, eps);
    bias[o] = (float)bn.bias;
    for (int i = 0; i < cin; ++i)
      for (int tap = 0; tap < taps; ++tap) {
        const float v = (float)ldexp((double)c.conv_w[((size_t)o * cin + i) * taps + tap] * bn.scale, S);
        const uint16_t hb = f32_to_f16_bits(v);
        const float hi = f16_bits_to_f32(hb);
        const uint16_t lb = f32_to_f16_bits(v - hi);
        uint8_t* row = &w[(size_t)o * KROW + ((size_t)tap * (cin / 64) + i / 64) * 256];
        memcpy(row + (i % 64) * 2, &hb, 2);
        if (q8) {
          row[128 + (i % 64)] = f32_to_e4m3(ldexpf(hi, kQ8WhiShift));
          row[192 + (i % 64)] = f32_to_e4m3(ldexpf(f16_bits_to_f32(lb), kQ8WloShift));
        } else {
          memcpy(row + 128 + (i % 64) * 2, &lb, 2);
        }
      }
  }
  const int rc = upload_convw(w.data(), w.size(), bias, out);
  out->wscale = ldexpf(1.f, S), out->winv = ldexpf(1.f, -S);
  return rc;
}

// Stem weights for the strip kernel (uint8 input, stem.h: stem_pool_strip2_kernel): BN folded as in
// pack_conv, ToTensor / Normalize (reference src/main.py:815-816) folded too -- the kernel feeds the centred byte
// value v - 128 (exact in bf16 and fp16; bytes outside the image arrive as 0, i.e. -128), so w'' = w * scale / (255 std_c)
// and the bias takes sum w'' (128 - mu''_c), mu''_c = 255 mean_c (the byte value of the normalised 0 the reference
// pads with), over the taps INSIDE the image and 128 sum w'' over the taps outside: one bias per (row class, column
// class) of the stem pixel, 16 x 64 floats.
// The fold uses the ROUNDED weights, so what is left of the weight rounding multiplies the centred value
// v - mu'', as in the unfolded form.
// K order: k = 16 s + 8 h + j, s = 4 c + rp, kh = 2 rp + (j & 1), kw = 4 h + (j >> 1); kh, kw = 7 are zero.
// Pair modes: w = the hi halves [64][192] followed by the lo halves [64][192] (fp16 pairs)
static int pack_stem_u8(const hipac_convbn_t& c, float eps, int precision, ConvW* out) {
  const double mean[3] = {0.485, 0.456, 0.406}, stdv[3] = {0.229, 0.224, 0.225};
  const bool split = pair_mode(precision);
  std::vector<uint16_t> w((size_t)64 * 192 * (split ? 2 : 1), 0);
  std::vector<float> tab((size_t)16 * 64 + 1);  // + tab[1024]: the factor that undoes the split weights' power-of-two scale
  // pair modes: the folded weights are ~1e-3 (w / (255 std)), whose lo halves would be fp16 subnormals (2^-24 quantum = only
  // 2^-15 of the weight): everything is scaled by 2^S (exact) so that the largest weight sits near 2^13, and the kernel
  // multiplies the pooled result by 2^-S
  double wscale = 1.0;
  if (split) {
    double wmax = 0.0;
    for (int o = 0; o < 64; ++o) {
      const double scale = bn_fold(c, o, eps).scale;
      for (int ch = 0; ch < 3; ++ch)
        for (int k = 0; k < 49; ++k) wmax = fmax(wmax, fabs((double)c.conv_w[((size_t)o * 3 + ch) * 49 + k] * scale / (255.0 * stdv[ch])));
    }
    int S = wmax > 0.0 ? (int)floor(log2(8192.0 / wmax)) : 0;
    S = S < 0 ? 0 : (S > 24 ? 24 : S);
    wscale = ldexp(1.0, S);
  }
  tab[16 * 64] = (float)(1.0 / wscale);
  double mu[3];
  for (int ch = 0; ch < 3; ++ch) mu[ch] = 255.0 * mean[ch];
  // taps of a stem pixel that fall outside the image, by class: 0 none, 1: row / column 0 (taps 0-2), 2: row / column 1
  // (tap 0), 3: row / column 111 (taps 5, 6)
  auto tap_out = [](int cls, int k) { return cls == 1 ? k <= 2 : (cls == 2 ? k == 0 : (cls == 3 ? k >= 5 : false)); };
  for (int o = 0; o < 64; ++o) {
    const BnFold bn = bn_fold(c, o, eps);
    double rw[3][7][7];  // rounded weights, as the kernel multiplies them
    for (int ch = 0; ch < 3; ++ch)
      for (int kh = 0; kh < 7; ++kh)
        for (int kw = 0; kw < 7; ++kw) {
          const double v = (double)c.conv_w[(((size_t)o * 3 + ch) * 7 + kh) * 7 + kw] * bn.scale / (255.0 * stdv[ch]) * wscale;
          const int s = 4 * ch + (kh >> 1), hq = kw >> 2, j = 2 * (kw & 3) + (kh & 1);
          if (split) {
            const float hi = round_to((float)v, HIPAC_PREC_FP16), lo = round_to((float)v - hi, HIPAC_PREC_FP16);
            w[(size_t)o * 192 + 16 * s + 8 * hq + j] = to_bits(hi, HIPAC_PREC_FP16);
            w[(size_t)(64 + o) * 192 + 16 * s + 8 * hq + j] = to_bits(lo, HIPAC_PREC_FP16);
            rw[ch][kh][kw] = (double)hi + (double)lo;
          } else {
            w[(size_t)o * 192 + 16 * s + 8 * hq + j] = to_bits((float)v, precision);
            rw[ch][kh][kw] = (double)round_to((float)v, precision);
          }
        }
    const double b0 = bn.bias * wscale;
    for (int rc = 0; rc < 4; ++rc)
      for (int cc = 0; cc < 4; ++cc) {
        // the kernel feeds v - 128 inside the image and 0 - 128 outside; the reference's sum is w (v - mu) over the
        // taps inside: bias + sum_inside w (128 - mu) + sum_outside 128 w
        double b = b0;
        for (int ch = 0; ch < 3; ++ch)
          for (int kh = 0; kh < 7; ++kh)
            for (int kw = 0; kw < 7; ++kw)
              b += (!tap_out(rc, kh) && !tap_out(cc, kw)) ? rw[ch][kh][kw] * (128.0 - mu[ch]) : rw[ch][kh][kw] * 128.0;
        tab[((size_t)rc * 4 + cc) * 64 + o] = (float)b;
      }
  }
  return upload_convw(w.data(), w.size() * 2, tab, out);
}

static void free_convw(ConvW& c) {
  if (c.w) (void)hipFree(c.w);
  if (c.bias) (void)hipFree(c.bias);
  c.w = nullptr;
  c.bias = nullptr;
}

#define PACK_TRY(expr)                      \
  do {                                      \
    if (const int rc__ = (expr)) return rc__; \
  } while (0)  // the failing step has set the error text

// Everything hipac_resnet18_pack uploads into the (zeroed) net; the caller frees the handle if this fails.
static int pack_net(const hipac_resnet18_params_t& params, int precision, Net& net) {
  net.precision = precision;
  net.num_classes = params.num_classes;
  net.projk = env_int("HIPAC_PROJK", 1, 0, 1);
  const float eps = params.bn_eps;
  const bool split = pair_mode(precision);
  const bool q8 = precision == HIPAC_PREC_FP16Q8;
  // Pair modes: the stem runs on the exact f32 MFMA (fp32 weights); all 16 block convs and the three projections are
  // packed as halo16x2.h's weight rows -- fp16q8 with e4m3 rows, fp16x3 with the lo halves as fp16.
  PACK_TRY(pack_conv(params.stem, 64, 3, 7, eps, split ? HIPAC_PREC_FP32 : precision, true, &net.stem));
  if (precision != HIPAC_PREC_FP32) PACK_TRY(pack_stem_u8(params.stem, eps, precision, &net.stem_u8));
  // pair modes: S < 0 = the conv's own power-of-two weight scale
  auto pack = [&](const hipac_convbn_t& c, int cout, int cin, int ks, ConvW* out, int S = -1) {
    if (!split) return pack_conv(c, cout, cin, ks, eps, precision, false, out);
    return pack_conv_pairs(c, cout, cin, ks * ks, eps, q8, S < 0 ? pair_shift(folded_absmax(c, cout, cin, ks * ks, eps)) : S, out);
  };
  const int ch[4] = {64, 128, 256, 512};
  int S_proj[3] = {-1, -1, -1};
  for (int s = 0; s < 4; ++s)
    for (int b = 0; b < 2; ++b)
      for (int k = 0; k < 2; ++k) {
        const int cin = s > 0 && b == 0 && k == 0 ? ch[s - 1] : ch[s];  // the stage's entry conv widens
        int S = -1;
        if (split && s > 0 && b == 0 && k == 1) {
          // the projection is folded into this conv (halo16x2.h, PCIN) and shares its accumulator: one S for the two
          const double wmax = fmax(folded_absmax(params.block[2 * s][1], ch[s], ch[s], 9, eps), folded_absmax(params.down[s - 1], ch[s], ch[s - 1], 1, eps));
          S = S_proj[s - 1] = pair_shift(wmax);
        }
        PACK_TRY(pack(params.block[2 * s + b][k], ch[s], cin, 3, &net.block[2 * s + b][k], S));
      }
  for (int s = 1; s < 4; ++s)  // (pair modes: folded into conv2, halo16x2.h, PCIN)
    PACK_TRY(pack(params.down[s - 1], ch[s], ch[s - 1], 1, &net.down[s - 1], S_proj[s - 1]));
  for (int s = 1; s < 4 && precision != HIPAC_PREC_FP32; ++s) {
    // block0.conv2's bias + the projection's, for the kernel that accumulates both into one accumulator
    std::vector<float> bs(ch[s]);
    for (int o = 0; o < ch[s]; ++o)
      bs[o] = (float)bn_fold(params.block[2 * s][1], o, eps).bias + (float)bn_fold(params.down[s - 1], o, eps).bias;
    PACK_TRY(upload(bs.data(), bs.size() * 4, (void**)&net.bias_c2p[s - 1]));
  }
  const char zeros[256] = {0};
  PACK_TRY(upload(zeros, sizeof(zeros), (void**)&net.zero_page));
  // ToTensor + Normalize table in fp32 with torchvision's op order (v/255, -mean, /std;
  // reference src/main.py:815-816), then rounded to the network's storage type
  const float mean[3] = {0.485f, 0.456f, 0.406f}, stdv[3] = {0.229f, 0.224f, 0.225f};
  std::vector<uint16_t> lut(3 * 256);
  std::vector<float> lutf(3 * 256);
  for (int c = 0; c < 3; ++c)
    for (int v = 0; v < 256; ++v) {
      const float t = (float)v / 255.0f;
      const float d = t - mean[c];
      lutf[c * 256 + v] = d / stdv[c];
      lut[c * 256 + v] = to_bits(d / stdv[c], wide_mode(precision) ? HIPAC_PREC_BF16 : precision);
    }
  PACK_TRY(upload(lut.data(), lut.size() * 2, (void**)&net.lut_t));
  PACK_TRY(upload(lutf.data(), lutf.size() * 4, (void**)&net.lut_f32));
  if (params.num_classes > 0) {
    PACK_TRY(upload(params.fc_w, (size_t)params.num_classes * 512 * 4, (void**)&net.fc_w));
    PACK_TRY(upload(params.fc_b, (size_t)params.num_classes * 4, (void**)&net.fc_b));
  }
  return 0;
}

}  // namespace hipac

using namespace hipac;

extern "C" {

void hipac_weights_free(hipac_weights_t* w) {
  if (!w) return;
  free_convw(w->net.stem);
  free_convw(w->net.stem_u8);
  for (int i = 0; i < 8; ++i)
    for (int j = 0; j < 2; ++j) free_convw(w->net.block[i][j]);
  for (int i = 0; i < 3; ++i) free_convw(w->net.down[i]);
  if (w->net.fc_w) (void)hipFree(w->net.fc_w);
  if (w->net.fc_b) (void)hipFree(w->net.fc_b);
  if (w->net.zero_page) (void)hipFree(w->net.zero_page);
  if (w->net.lut_t) (void)hipFree(w->net.lut_t);
  if (w->net.lut_f32) (void)hipFree(w->net.lut_f32);
  for (int i = 0; i < 3; ++i)
    if (w->net.bias_c2p[i]) (void)hipFree(w->net.bias_c2p[i]);
  for (hipStream_t s : w->lane_stream)
    if (s) (void)hipStreamDestroy(s);
  delete w;
}

int hipac_resnet18_pack(const hipac_resnet18_params_t* params, int precision, hipac_weights_t** out) {
  HIPAC_REQUIRE(params && out, HIPAC_EINVAL, "pack: null argument");
  HIPAC_REQUIRE(precision == HIPAC_PREC_BF16 || precision == HIPAC_PREC_FP16 || precision == HIPAC_PREC_FP32 ||
                    precision == HIPAC_PREC_FP16X3 || precision == HIPAC_PREC_FP16Q8,
                HIPAC_EINVAL, "pack: unknown precision %d", precision);
  HIPAC_REQUIRE(params->num_classes >= 0 && params->num_classes <= 16, HIPAC_EINVAL,
                "pack: num_classes %d out of range", params->num_classes);
  HIPAC_REQUIRE((params->num_classes == 0) == (params->fc_w == nullptr), HIPAC_EINVAL,
                "pack: fc_w / num_classes mismatch");
  HIPAC_REQUIRE(params->num_classes == 0 || params->fc_b != nullptr, HIPAC_EINVAL, "pack: fc_b is null");
  int device = 0;
  HIPAC_CHECK_HIP(hipGetDevice(&device));
  // from here on every failure goes through hipac_weights_free
  hipac_weights_t* w = new hipac_weights_t();
  memset(&w->net, 0, sizeof(Net));
  w->device = device;
  const int rc = pack_net(*params, precision, w->net);
  if (rc) {
    hipac_weights_free(w);
    return rc;
  }
  // optional: without them forward simply runs single-lane
  for (hipStream_t& s : w->lane_stream)
    if (hipStreamCreateWithFlags(&s, hipStreamNonBlocking) != hipSuccess) s = nullptr;
  *out = w;
  return 0;
}

int hipac_weights_precision(const hipac_weights_t* w) { return w ? w->net.precision : HIPAC_EINVAL; }
int hipac_weights_num_classes(const hipac_weights_t* w) { return w ? w->net.num_classes : HIPAC_EINVAL; }

}  // extern "C"
