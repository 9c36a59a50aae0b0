// Host-side checks of nft_mirror_mix and the nft_prod_* entry points under
// AddressSanitizer (the pattern of matern_host_driver.cpp): sizing arithmetic
// and the argument validation that rejects a call before any launch.  The
// host code is built with -fsanitize=address; no call here reaches the device.
// Exit code 0 = every check held and ASan reported nothing.
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

int main() {
  // sizing: z, z ls_o and the two quotient vectors padded to even lengths;
  // row partials per column tile of 256, column partials per row tile of 16,
  // one full partial per tile, padded to an even count
  CHECK(nft_prod_const_size(1, 5) == 0 && nft_prod_const_size(5, 1) == 0 && nft_prod_workspace(1, 5) == 0);
  CHECK(nft_prod_const_size(2, 2) == 6 && nft_prod_const_size(9, 5) == 18 && nft_prod_const_size(65, 33) == 102);
  CHECK(nft_prod_workspace(9, 5) == (9 + 5 + 1 + 1) * sizeof(double));            // one tile
  CHECK(nft_prod_workspace(65, 33) == (65 + 5 * 33 + 5 + 1) * sizeof(double));    // 5 row tiles
  CHECK(nft_prod_workspace(3, 513) == (3 * 3 + 513 + 3 + 1) * sizeof(double));    // 3 column tiles
  CHECK(nft_prod_workspace(20000, 17) == (20000 + 1250 * 17 + 1250) * sizeof(double));

  double dummy[8] = {0};
  // mirror mix
  {
    const int64_t s2[2] = {4, 8}, s3[3] = {4, 6, 8}, s0[2] = {4, 0}, s4[4] = {2, 2, 2, 2};
    CHECK(nft_mirror_mix(nullptr, 32, dummy, 32, 1, 2, s2, 1, 0, nullptr) == NFT_ERR_ARG);
    CHECK(err_mentions("nft_mirror_mix"));
    CHECK(nft_mirror_mix(dummy, 32, nullptr, 32, 1, 2, s2, 1, 0, nullptr) == NFT_ERR_ARG);
    CHECK(nft_mirror_mix(dummy, 32, dummy, 32, 1, 2, nullptr, 1, 0, nullptr) == NFT_ERR_ARG);
    CHECK(nft_mirror_mix(dummy, 32, dummy, 32, 0, 2, s2, 1, 0, nullptr) == NFT_ERR_ARG);   // no row
    CHECK(nft_mirror_mix(dummy, 32, dummy, 32, 1, 1, s2, 1, 0, nullptr) == NFT_ERR_ARG);   // one axis: no two groups
    CHECK(nft_mirror_mix(dummy, 32, dummy, 32, 1, 4, s4, 2, 0, nullptr) == NFT_ERR_ARG);
    CHECK(nft_mirror_mix(dummy, 32, dummy, 32, 1, 2, s2, 0, 0, nullptr) == NFT_ERR_ARG);   // empty group 1
    CHECK(nft_mirror_mix(dummy, 32, dummy, 32, 1, 2, s2, 2, 0, nullptr) == NFT_ERR_ARG);   // empty group 2
    CHECK(nft_mirror_mix(dummy, 192, dummy, 192, 1, 3, s3, 3, 0, nullptr) == NFT_ERR_ARG);
    CHECK(nft_mirror_mix(dummy, 32, dummy, 32, 1, 2, s0, 1, 0, nullptr) == NFT_ERR_ARG);   // axis of length 0
    CHECK(nft_mirror_mix(dummy, 32, dummy, 32, 1, 2, s2, 1, 2, nullptr) == NFT_ERR_ARG);   // dtype
    CHECK(nft_mirror_mix(dummy, 31, dummy + 1, 32, 2, 2, s2, 1, 0, nullptr) == NFT_ERR_ARG);  // x rows overlap
    CHECK(nft_mirror_mix(dummy, 32, dummy + 1, 31, 2, 2, s2, 1, 0, nullptr) == NFT_ERR_ARG);  // y rows overlap
    CHECK(nft_mirror_mix(dummy, 32, dummy, 40, 1, 2, s2, 1, 0, nullptr) == NFT_ERR_ARG);   // in place, strides differ
    CHECK(nft_mirror_mix(dummy, -1, dummy + 1, 32, 1, 2, s2, 1, 0, nullptr) == NFT_ERR_ARG);
  }
  // forward
  {
    CHECK(nft_prod_forward(1, 5, dummy, 0, dummy, 0, dummy, 0, 0., 1., 1., 1., 1., 1, dummy, 5, dummy, 18, nullptr) ==
          NFT_ERR_ARG);
    CHECK(err_mentions("nft_prod_forward"));
    CHECK(nft_prod_forward(9, 1, dummy, 0, dummy, 0, dummy, 0, 0., 1., 1., 1., 1., 1, dummy, 9, dummy, 18, nullptr) ==
          NFT_ERR_ARG);
    CHECK(nft_prod_forward(9, 5, nullptr, 0, dummy, 0, dummy, 0, 0., 1., 1., 1., 1., 1, dummy, 45, dummy, 18,
                           nullptr) == NFT_ERR_ARG);
    CHECK(nft_prod_forward(9, 5, dummy, 0, nullptr, 0, dummy, 0, 0., 1., 1., 1., 1., 1, dummy, 45, dummy, 18,
                           nullptr) == NFT_ERR_ARG);
    CHECK(nft_prod_forward(9, 5, dummy, 0, dummy, 0, nullptr, 0, 0., 1., 1., 1., 1., 1, dummy, 45, dummy, 18,
                           nullptr) == NFT_ERR_ARG);
    CHECK(nft_prod_forward(9, 5, dummy, 0, dummy, 0, dummy, 0, 0., 1., 1., 1., 1., 1, nullptr, 45, dummy, 18,
                           nullptr) == NFT_ERR_ARG);
    CHECK(nft_prod_forward(9, 5, dummy, 0, dummy, 0, dummy, 0, 0., 1., 1., 1., 1., 1, dummy, 45, nullptr, 18,
                           nullptr) == NFT_ERR_ARG);
    CHECK(nft_prod_forward(9, 5, dummy, 0, dummy, 0, dummy, 0, 0., 1., 1., 1., 1., 0, dummy, 45, dummy, 18,
                           nullptr) == NFT_ERR_ARG);  // no item
    CHECK(nft_prod_forward(9, 5, dummy, 0, dummy, 0, dummy, 0, 0., 1., 0., 1., 1., 1, dummy, 45, dummy, 18,
                           nullptr) == NFT_ERR_ARG);  // s0 = 0
    CHECK(nft_prod_forward(9, 5, dummy, 9, dummy, 5, dummy, 1, 0., 1., 1., 1., 1., 2, dummy, 44, dummy, 18,
                           nullptr) == NFT_ERR_ARG);  // rows of A overlap
    CHECK(nft_prod_forward(9, 5, dummy, 9, dummy, 5, dummy, 1, 0., 1., 1., 1., 1., 2, dummy, 45, dummy, 17,
                           nullptr) == NFT_ERR_ARG);  // constant sets overlap
    CHECK(nft_prod_forward(9, 5, dummy, -9, dummy, 5, dummy, 1, 0., 1., 1., 1., 1., 2, dummy, 45, dummy, 18,
                           nullptr) == NFT_ERR_ARG);
  }
  // JVP
  {
    CHECK(nft_prod_jvp_batched(1, 5, dummy, 1., 1., dummy, 9, dummy, 5, dummy, 8, dummy, 4, nullptr) == NFT_ERR_ARG);
    CHECK(err_mentions("nft_prod_jvp_batched"));
    CHECK(nft_prod_jvp_batched(9, 5, nullptr, 1., 1., dummy, 9, dummy, 5, dummy, 8, dummy, 4, nullptr) == NFT_ERR_ARG);
    CHECK(nft_prod_jvp_batched(9, 5, dummy, 1., 1., nullptr, 9, dummy, 5, dummy, 8, dummy, 4, nullptr) == NFT_ERR_ARG);
    CHECK(nft_prod_jvp_batched(9, 5, dummy, 1., 1., dummy, 9, nullptr, 5, dummy, 8, dummy, 4, nullptr) == NFT_ERR_ARG);
    CHECK(nft_prod_jvp_batched(9, 5, dummy, 1., 1., dummy, 9, dummy, 5, nullptr, 8, dummy, 4, nullptr) == NFT_ERR_ARG);
    CHECK(nft_prod_jvp_batched(9, 5, dummy, 1., 1., dummy, 9, dummy, 5, dummy, 8, nullptr, 4, nullptr) == NFT_ERR_ARG);
    CHECK(nft_prod_jvp_batched(9, 5, dummy, 1., 1., dummy, 9, dummy, 5, dummy, 8, dummy, 0, nullptr) == NFT_ERR_ARG);
    CHECK(nft_prod_jvp_batched(9, 5, dummy, 1., 1., dummy, 8, dummy, 5, dummy, 8, dummy, 4, nullptr) == NFT_ERR_ARG);
    CHECK(nft_prod_jvp_batched(9, 5, dummy, 1., 1., dummy, 9, dummy, 4, dummy, 8, dummy, 4, nullptr) == NFT_ERR_ARG);
    CHECK(nft_prod_jvp_batched(9, 5, dummy, 1., 1., dummy, 9, dummy, 5, dummy, -8, dummy, 4, nullptr) == NFT_ERR_ARG);
  }
  // VJP
  {
    CHECK(nft_prod_vjp_batched(9, 1, dummy, 1., 1., dummy, 45, dummy, 9, dummy, 5, dummy, nullptr, 8, 0., dummy, 4,
                               nullptr) == NFT_ERR_ARG);
    CHECK(err_mentions("nft_prod_vjp_batched"));
    CHECK(nft_prod_vjp_batched(9, 5, nullptr, 1., 1., dummy, 45, dummy, 9, dummy, 5, dummy, nullptr, 8, 0., dummy, 4,
                               nullptr) == NFT_ERR_ARG);
    CHECK(nft_prod_vjp_batched(9, 5, dummy, 1., 1., nullptr, 45, dummy, 9, dummy, 5, dummy, nullptr, 8, 0., dummy, 4,
                               nullptr) == NFT_ERR_ARG);
    CHECK(nft_prod_vjp_batched(9, 5, dummy, 1., 1., dummy, 45, nullptr, 9, dummy, 5, dummy, nullptr, 8, 0., dummy, 4,
                               nullptr) == NFT_ERR_ARG);
    CHECK(nft_prod_vjp_batched(9, 5, dummy, 1., 1., dummy, 45, dummy, 9, nullptr, 5, dummy, nullptr, 8, 0., dummy, 4,
                               nullptr) == NFT_ERR_ARG);
    CHECK(nft_prod_vjp_batched(9, 5, dummy, 1., 1., dummy, 45, dummy, 9, dummy, 5, nullptr, nullptr, 8, 0., dummy, 4,
                               nullptr) == NFT_ERR_ARG);
    CHECK(nft_prod_vjp_batched(9, 5, dummy, 1., 1., dummy, 45, dummy, 9, dummy, 5, dummy, nullptr, 8, 0., nullptr, 4,
                               nullptr) == NFT_ERR_ARG);  // no workspace
    CHECK(nft_prod_vjp_batched(9, 5, dummy, 1., 1., dummy, 45, dummy, 9, dummy, 5, dummy, nullptr, 8, 0., dummy, 0,
                               nullptr) == NFT_ERR_ARG);  // nrhs 0
    CHECK(nft_prod_vjp_batched(9, 5, dummy, 1., 1., dummy, 44, dummy, 9, dummy, 5, dummy, nullptr, 8, 0., dummy, 4,
                               nullptr) == NFT_ERR_ARG);  // g rows overlap
    CHECK(nft_prod_vjp_batched(9, 5, dummy, 1., 1., dummy, 45, dummy, 8, dummy, 5, dummy, nullptr, 8, 0., dummy, 4,
                               nullptr) == NFT_ERR_ARG);  // gm1 rows overlap
    CHECK(nft_prod_vjp_batched(9, 5, dummy, 1., 1., dummy, 45, dummy, 9, dummy, 4, dummy, nullptr, 8, 0., dummy, 4,
                               nullptr) == NFT_ERR_ARG);  // gm2 rows overlap
    CHECK(nft_prod_vjp_batched(9, 5, dummy, 1., 1., dummy, 45, dummy, 9, dummy, 5, dummy, nullptr, 0, 0., dummy, 4,
                               nullptr) == NFT_ERR_ARG);  // zero-mode outputs overlap
    CHECK(nft_prod_vjp_batched(16 * 65535 + 1, 5, dummy, 1., 1., dummy, 0, dummy, 0, dummy, 0, dummy, nullptr, 0, 0.,
                               dummy, 1, nullptr) == NFT_ERR_ARG);  // more row tiles than a launch takes
  }
  CHECK(std::strlen(nft_last_error()) < 4096);
  if (fails) {
    std::fprintf(stderr, "%d check(s) failed\n", fails);
    return 1;
  }
  std::printf("product host checks: ok\n");
  return 0;
}
