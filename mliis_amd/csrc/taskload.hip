// libmliis_data.so: a task's shots made resident from the bytes a dataset stores (include/mliis_data.h).  A library of its own beside
// libmliis_hip.so and libmliis_score.so -- the training step's library and its C ABI (include/mliis_hip.h) are untouched by it.
// Reference: data/input_fn.py:28-65 (image -> float32 0..255, mask -> (255 - m, m) / 255); the resampling the reference's docstring
// promises and its code does not have (it reshapes) is stated in the header.
#include "../../include/mliis_data.h"
#include "common.hpp"

namespace mliis {

// (this library's own error slot: common.hpp's MLIIS_REQUIRE / MLIIS_CHECK_LAUNCH report through set_error of the library they are linked into)
MLIIS_DEFINE_ERROR_SLOT(g_data_err)

// k / 255 correctly rounded in fp32 for the 256 byte values: evaluated by the compiler (IEEE round to nearest), so the label values do
// not depend on how the device divides.  numpy's float32 division gives the same 256 floats (tests/test_taskload_cpu.py).
struct ByteQuotients {
  float v[256];
};
constexpr ByteQuotients make_byte_quotients() {
  ByteQuotients t{};
  for (int k = 0; k < 256; ++k) t.v[k] = (float)k / 255.0f;
  return t;
}
__constant__ const ByteQuotients k_q255 = make_byte_quotients();

// The kernel is a stream: per output pixel 20 bytes written, 4 (same size) or about 16 (resampled) read.  The outputs are taken as FLAT
// pixel arrays [S*H*W][3] and [S*H*W][2] and a thread owns four consecutive flat pixels p0 .. p0 + 3, p0 a multiple of 4: its 12 + 8
// floats start at byte 48 (p0/4) of x and 32 (p0/4) of y, so with 16-byte aligned x / y every store of a full group is a 16-byte store
// whatever W and H are (7 x 7 images, 21-byte source rows); a group may straddle rows and images -- each pixel finds its own (image, row,
// column) -- and only the last group of the whole tensor can be short (scalar stores).  No LDS, no traffic between workgroups; the index
// vector is read through the scalar / L1 path (a workgroup covers 1024 pixels: one or two images).
//   MODE 0: same size, pool 4-byte aligned and h w % 4 == 0: a group lies in one image at a 4-byte aligned source offset -- three
//           word loads for its 12 image bytes, one for its 4 mask bytes.
//   MODE 1: same size, byte loads (any alignment, any pitch).
//   MODE 2: resampled (header: nearest mask, bilinear image at half-pixel centres, integer coordinates).
__device__ __forceinline__ int clamp_row(const int* __restrict__ idx, int s, int n) {
  const int r = idx ? idx[s] : s;
  return min(max(r, 0), n - 1);
}

__device__ __forceinline__ void label_pair(unsigned m, float* __restrict__ yv) {
  yv[0] = k_q255.v[255u - m];
  yv[1] = k_q255.v[m];
}

// integer half-pixel coordinates of output index i (size O) in a source of size I: the two taps and the fraction, no rounding in them
__device__ __forceinline__ void taps(int i, int I, int O, int& i0, int& i1, float& f) {
  const int den = 2 * O;
  const int num = min(max((2 * i + 1) * I - O, 0), den * (I - 1));
  i0 = num / den;
  i1 = min(i0 + 1, I - 1);
  f = (float)(num - i0 * den) / (float)den;
}

template <int MODE>
__global__ __launch_bounds__(256) void task_expand_u8_k(const unsigned char* __restrict__ images, const unsigned char* __restrict__ masks,
                                                        const int* __restrict__ idx, unsigned P, int n, int h, int w, int H, int W,
                                                        float* __restrict__ x, float* __restrict__ y) {
  const unsigned g = blockIdx.x * 256u + threadIdx.x;
  if (g >= (P + 3u) / 4u) return;
  const unsigned p0 = g * 4u;
  const unsigned HW = (unsigned)H * (unsigned)W;
  const int cnt = (int)min(4u, P - p0);
  float xv[12], yv[8];
  if (MODE == 0) {   // (cnt == 4 always: P is a multiple of 4 here)
    const unsigned s = p0 / HW, q = p0 - s * HW;
    const long long src = (long long)clamp_row(idx, (int)s, n) * HW + q;
    const unsigned* ip = reinterpret_cast<const unsigned*>(images + src * 3);
    const unsigned i0 = ip[0], i1 = ip[1], i2 = ip[2];
    const unsigned mm = *reinterpret_cast<const unsigned*>(masks + src);
#pragma unroll
    for (int b = 0; b < 4; ++b) {
      xv[b] = (float)((i0 >> (8 * b)) & 255u);
      xv[4 + b] = (float)((i1 >> (8 * b)) & 255u);
      xv[8 + b] = (float)((i2 >> (8 * b)) & 255u);
      label_pair((mm >> (8 * b)) & 255u, yv + 2 * b);
    }
  } else {
    const long long hw = (long long)h * w;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      if (k < cnt) {
        const unsigned p = p0 + k;
        const unsigned s = p / HW, r = p - s * HW;
        const long long base = (long long)clamp_row(idx, (int)s, n) * hw;
        if (MODE == 1) {
          const unsigned char* ip = images + (base + r) * 3;
          xv[3 * k] = (float)ip[0];
          xv[3 * k + 1] = (float)ip[1];
          xv[3 * k + 2] = (float)ip[2];
          label_pair(masks[base + r], yv + 2 * k);
        } else {
          const int i = (int)(r / (unsigned)W), j = (int)(r - (unsigned)i * (unsigned)W);
          const int mi = ((2 * i + 1) * h) / (2 * H), mj = ((2 * j + 1) * w) / (2 * W);
          label_pair(masks[base + (long long)mi * w + mj], yv + 2 * k);
          int i0, i1, j0, j1;
          float fy, fx;
          taps(i, h, H, i0, i1, fy);
          taps(j, w, W, j0, j1, fx);
          const unsigned char* r0 = images + (base + (long long)i0 * w) * 3;
          const unsigned char* r1 = images + (base + (long long)i1 * w) * 3;
#pragma unroll
          for (int c = 0; c < 3; ++c) {
            const float a00 = (float)r0[3 * j0 + c], a01 = (float)r0[3 * j1 + c];
            const float a10 = (float)r1[3 * j0 + c], a11 = (float)r1[3 * j1 + c];
            const float top = a00 + (a01 - a00) * fx;
            const float bot = a10 + (a11 - a10) * fx;
            xv[3 * k + c] = top + (bot - top) * fy;
          }
        }
      }
    }
  }
  float* xo = x + (long long)p0 * 3;
  float* yo = y + (long long)p0 * 2;
  if (cnt == 4) {
    float4* x4 = reinterpret_cast<float4*>(xo);
    float4* y4 = reinterpret_cast<float4*>(yo);
    x4[0] = make_float4(xv[0], xv[1], xv[2], xv[3]);
    x4[1] = make_float4(xv[4], xv[5], xv[6], xv[7]);
    x4[2] = make_float4(xv[8], xv[9], xv[10], xv[11]);
    y4[0] = make_float4(yv[0], yv[1], yv[2], yv[3]);
    y4[1] = make_float4(yv[4], yv[5], yv[6], yv[7]);
  } else {
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      if (k < cnt) {
        xo[3 * k] = xv[3 * k];
        xo[3 * k + 1] = xv[3 * k + 1];
        xo[3 * k + 2] = xv[3 * k + 2];
        yo[2 * k] = yv[2 * k];
        yo[2 * k + 1] = yv[2 * k + 1];
      }
    }
  }
}

}  // namespace mliis

using namespace mliis;

extern "C" {

const char* mliis_data_last_error(void) { return g_data_err; }

// include/mliis_data.h.  One launch.
int mliis_task_expand_u8(const unsigned char* images, const unsigned char* masks, const int* src_idx, int S, int n, int h, int w, int H,
                         int W, float* x, float* y, hipStream_t stream) {
  MLIIS_REQUIRE(images, MLIIS_ERR_ARG, "task_expand_u8: images is null");
  MLIIS_REQUIRE(masks, MLIIS_ERR_ARG, "task_expand_u8: masks is null");
  MLIIS_REQUIRE(x, MLIIS_ERR_ARG, "task_expand_u8: x is null");
  MLIIS_REQUIRE(y, MLIIS_ERR_ARG, "task_expand_u8: y is null");
  MLIIS_REQUIRE(S >= 1, MLIIS_ERR_ARG, "task_expand_u8: S = %d (at least one example)", S);
  MLIIS_REQUIRE(n >= 1, MLIIS_ERR_ARG, "task_expand_u8: n = %d (the pool holds at least one example)", n);
  MLIIS_REQUIRE(h >= 1, MLIIS_ERR_ARG, "task_expand_u8: h = %d", h);
  MLIIS_REQUIRE(w >= 1, MLIIS_ERR_ARG, "task_expand_u8: w = %d", w);
  MLIIS_REQUIRE(H >= 1, MLIIS_ERR_ARG, "task_expand_u8: H = %d", H);
  MLIIS_REQUIRE(W >= 1, MLIIS_ERR_ARG, "task_expand_u8: W = %d", W);
  MLIIS_REQUIRE(aligned16(x), MLIIS_ERR_ALIGN, "task_expand_u8: x must be 16-byte aligned");
  MLIIS_REQUIRE(aligned16(y), MLIIS_ERR_ALIGN, "task_expand_u8: y must be 16-byte aligned");
  MLIIS_REQUIRE(h <= 16384 && w <= 16384 && H <= 16384 && W <= 16384, MLIIS_ERR_UNSUPPORTED,
                "task_expand_u8: h, w, H, W up to 16384 (the half-pixel coordinates are 32-bit integers)");
  const long long P = (long long)S * H * W;
  MLIIS_REQUIRE(P <= 0x7fffffffLL, MLIIS_ERR_UNSUPPORTED, "task_expand_u8: S * H * W = %lld output pixels (up to 2^31 - 1)", P);
  const dim3 grid(ceil_div((P + 3) / 4, 256)), block(256);
  const bool same = h == H && w == W;
  const bool words = same && ((long long)h * w) % 4 == 0 && (reinterpret_cast<uintptr_t>(images) & 3u) == 0 &&
                     (reinterpret_cast<uintptr_t>(masks) & 3u) == 0;
  if (words)
    hipLaunchKernelGGL(task_expand_u8_k<0>, grid, block, 0, stream, images, masks, src_idx, (unsigned)P, n, h, w, H, W, x, y);
  else if (same)
    hipLaunchKernelGGL(task_expand_u8_k<1>, grid, block, 0, stream, images, masks, src_idx, (unsigned)P, n, h, w, H, W, x, y);
  else
    hipLaunchKernelGGL(task_expand_u8_k<2>, grid, block, 0, stream, images, masks, src_idx, (unsigned)P, n, h, w, H, W, x, y);
  MLIIS_CHECK_LAUNCH("task_expand_u8");
  return MLIIS_OK;
}
}
