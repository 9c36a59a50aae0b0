// Host-side checks of the nft_conv_space_* entry points under AddressSanitizer
// (the pattern of product_host_driver.cpp): the supported-domain table, the
// sizing arithmetic and the argument validation that rejects a call before
// any launch.  The host code is built with -fsanitize=address; no call here
// reaches the device.  Exit code 0 = every check held and ASan reported
// nothing.
#include <cstdio>
#include <cstring>

#include "nifty_amd.h"

static int fails = 0;
#define CHECK(c)                                                          \
  do {                                                                    \
    if (!(c)) {                                                           \
      std::fprintf(stderr, "FAILED %s:%d: %s\n", __FILE__, __LINE__, #c); \
      ++fails;                                                            \
    }                                                                     \
  } while (0)

static bool err_mentions(const char* s) {
  const char* e = nft_last_error();
  return e && std::strstr(e, s) != nullptr;
}

static size_t up256(size_t b) { return (b + 255) & ~(size_t)255; }

int main() {
  // supported domains: fp64, n1 8..512, n0 8..512 or 1024..16384, powers of
  // two, ne even, fewer than 2^31 pixels
  CHECK(nft_conv_space_supported(8, 8, 4, 0) == 1 && nft_conv_space_supported(16, 8, 2, 0) == 1);
  CHECK(nft_conv_space_supported(8, 512, 10, 0) == 1 && nft_conv_space_supported(1024, 8, 2, 0) == 1);
  CHECK(nft_conv_space_supported(512, 512, 32, 0) == 1 && nft_conv_space_supported(16384, 8, 2, 0) == 1);
  CHECK(nft_conv_space_supported(8, 8, 4, 1) == 0);                                             // fp32
  CHECK(nft_conv_space_supported(8, 8, 5, 0) == 0 && nft_conv_space_supported(8, 8, 0, 0) == 0);   // odd, empty
  CHECK(nft_conv_space_supported(8, 8, -2, 0) == 0 && nft_conv_space_supported(-8, 8, 2, 0) == 0);
  CHECK(nft_conv_space_supported(8, 6, 4, 0) == 0 && nft_conv_space_supported(6, 8, 4, 0) == 0);
  CHECK(nft_conv_space_supported(4, 8, 2, 0) == 0 && nft_conv_space_supported(8, 4, 2, 0) == 0);
  CHECK(nft_conv_space_supported(8, 1024, 2, 0) == 0 && nft_conv_space_supported(32768, 8, 2, 0) == 0);
  CHECK(nft_conv_space_supported(768, 8, 2, 0) == 0);
  CHECK(nft_conv_space_supported(16384, 512, 256, 0) == 0);                                     // 2^31 pixels
  CHECK(nft_conv_space_supported(8, 8, (int64_t)1 << 40, 0) == 0);

  double dummy[8] = {0};
  nft_conv_space_plan p = {8, 512, 5, dummy, 1.5};
  // sizing: the complex grids, one mean partial per tile of 2048 / n1 lines,
  // one mean term per vector, each padded to 256 bytes
  CHECK(nft_conv_space_quad_blocks(&p) == 10);
  CHECK(nft_conv_space_workspace(&p, 1) == up256(8 * 512 * 5 * 16) + up256(10 * 8) + up256(8));
  CHECK(nft_conv_space_workspace(&p, 9) == up256(9 * 8 * 512 * 5 * 16) + up256(9 * 10 * 8) + up256(9 * 8));
  CHECK(nft_conv_space_workspace(&p, 0) == 0 && nft_conv_space_workspace(nullptr, 1) == 0);
  CHECK(nft_conv_space_quad_blocks(nullptr) == 0);
  {
    nft_conv_space_plan q = {8, 8, 2, dummy, 1.0};
    CHECK(nft_conv_space_quad_blocks(&q) == 1);     // 16 lines in one tile of 256
    q.inner = 3;
    CHECK(nft_conv_space_quad_blocks(&q) == 1);
    q.n0 = 1024;
    q.inner = 1;
    CHECK(nft_conv_space_quad_blocks(&q) == 4);
    q.n1 = 6;                                       // not served
    CHECK(nft_conv_space_quad_blocks(&q) == 0);
  }
  const int64_t P = 8 * 512 * 10;
  const size_t need = nft_conv_space_workspace(&p, 2);
  // bad plans
  {
    nft_conv_space_plan q = p;
    q.table = nullptr;
    CHECK(nft_conv_space_workspace(&q, 1) == 0 && nft_conv_space_quad_blocks(&q) == 0);
    CHECK(nft_conv_space_apply_batched(&q, dummy, P, nullptr, dummy, P, nullptr, 1., 1, 0, nullptr, 0, dummy, need,
                                       nullptr) == NFT_ERR_ARG);
    CHECK(err_mentions("conv space: bad plan"));
    q = p;
    q.n0 = 0;
    CHECK(nft_conv_space_apply_batched(&q, dummy, P, nullptr, dummy, P, nullptr, 1., 1, 0, nullptr, 0, dummy, need,
                                       nullptr) == NFT_ERR_ARG);
    q = p;
    q.n1 = -8;
    CHECK(nft_conv_space_apply_batched(&q, dummy, P, nullptr, dummy, P, nullptr, 1., 1, 0, nullptr, 0, dummy, need,
                                       nullptr) == NFT_ERR_ARG);
    q = p;
    q.inner = 0;
    CHECK(nft_conv_space_apply_batched(&q, dummy, P, nullptr, dummy, P, nullptr, 1., 1, 0, nullptr, 0, dummy, need,
                                       nullptr) == NFT_ERR_ARG);
    CHECK(nft_conv_space_apply_batched(nullptr, dummy, P, nullptr, dummy, P, nullptr, 1., 1, 0, nullptr, 0, dummy,
                                       need, nullptr) == NFT_ERR_ARG);
  }
  // NULL vectors, no vector
  CHECK(nft_conv_space_apply_batched(&p, nullptr, P, nullptr, dummy, P, nullptr, 1., 1, 0, nullptr, 0, dummy, need,
                                     nullptr) == NFT_ERR_ARG);
  CHECK(err_mentions("NULL vector"));
  CHECK(nft_conv_space_apply_batched(&p, dummy, P, nullptr, nullptr, P, nullptr, 1., 1, 0, nullptr, 0, dummy, need,
                                     nullptr) == NFT_ERR_ARG);
  CHECK(nft_conv_space_apply_batched(&p, dummy, P, nullptr, dummy, P, nullptr, 1., 0, 0, nullptr, 0, dummy, need,
                                     nullptr) == NFT_ERR_ARG);
  // unsupported shapes and dtype
  {
    nft_conv_space_plan q = p;
    q.n1 = 6;
    CHECK(nft_conv_space_apply_batched(&q, dummy, P, nullptr, dummy, P, nullptr, 1., 1, 0, nullptr, 0, dummy, need,
                                       nullptr) == NFT_ERR_UNSUPPORTED);
    CHECK(err_mentions("nft_conv_space_supported"));
    q = p;
    q.n0 = 768;
    CHECK(nft_conv_space_apply_batched(&q, dummy, 768 * P, nullptr, dummy, 768 * P, nullptr, 1., 1, 0, nullptr, 0,
                                       dummy, need, nullptr) == NFT_ERR_UNSUPPORTED);
    q = p;
    q.inner = (int64_t)1 << 40;
    CHECK(nft_conv_space_apply_batched(&q, dummy, P, nullptr, dummy, P, nullptr, 1., 1, 0, nullptr, 0, dummy, need,
                                       nullptr) == NFT_ERR_UNSUPPORTED);
    CHECK(nft_conv_space_workspace(&q, 1) == 0 && nft_conv_space_quad_blocks(&q) == 0);
    CHECK(nft_conv_space_apply_batched(&p, dummy, P, nullptr, dummy, P, nullptr, 1., 1, 1, nullptr, 0, dummy, need,
                                       nullptr) == NFT_ERR_UNSUPPORTED);   // fp32
  }
  // short strides
  CHECK(nft_conv_space_apply_batched(&p, dummy, P - 1, nullptr, dummy, P, nullptr, 1., 2, 0, nullptr, 0, dummy, need,
                                     nullptr) == NFT_ERR_ARG);
  CHECK(err_mentions("strides"));
  CHECK(nft_conv_space_apply_batched(&p, dummy, P, nullptr, dummy, P - 1, nullptr, 1., 2, 0, nullptr, 0, dummy, need,
                                     nullptr) == NFT_ERR_ARG);
  CHECK(nft_conv_space_apply_batched(&p, dummy, -P, nullptr, dummy, P, nullptr, 1., 2, 0, nullptr, 0, dummy, need,
                                     nullptr) == NFT_ERR_ARG);
  // short qstride
  CHECK(nft_conv_space_apply_batched(&p, dummy, P, nullptr, dummy, P, nullptr, 1., 2, 0, dummy, 9, dummy, need,
                                     nullptr) == NFT_ERR_ARG);
  CHECK(err_mentions("qstride"));
  // short or missing workspace
  CHECK(nft_conv_space_apply_batched(&p, dummy, P, nullptr, dummy, P, nullptr, 1., 2, 0, dummy, 10, dummy, need - 1,
                                     nullptr) == NFT_ERR_ARG);
  CHECK(err_mentions("workspace"));
  CHECK(nft_conv_space_apply_batched(&p, dummy, P, nullptr, dummy, P, nullptr, 1., 2, 0, dummy, 10, nullptr, need,
                                     nullptr) == NFT_ERR_ARG);
  CHECK(std::strlen(nft_last_error()) < 4096);
  if (fails) {
    std::fprintf(stderr, "%d check(s) failed\n", fails);
    return 1;
  }
  std::printf("conv space host checks: ok\n");
  return 0;
}
