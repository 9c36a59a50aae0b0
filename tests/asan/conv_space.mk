# AddressSanitizer build of the library's HOST code (as product.mk beside this
# file: -fsanitize applies to the host side only, device code is compiled as
# usual) with csrc/nft_conv.hip, and the host-only driver of the
# nft_conv_space_* argument checks.  Objects are shared with Makefile's and
# product.mk's in build/.
#   make -C tests/asan -f conv_space.mk && ./tests/asan/build/conv_space_host_driver
HIPCC ?= /opt/rocm/bin/hipcc
ARCH ?= gfx950
CSRC := ../../joss-nifty_amd/csrc
SAN := -Xarch_host -fsanitize=address -Xarch_host -fno-omit-frame-pointer
CXXFLAGS := -O1 -g -std=c++17 -fPIC --offload-arch=$(ARCH) -I../../include -w $(SAN)
SRCS := nft_fft nft_pro_r2c nft_blas nft_cf nft_spmv nft_amp nft_amp2 nft_matern nft_prod nft_los nft_samp nft_conv \
        nft_prof nft_lh
OBJS := $(SRCS:%=build/%.o)

all: build/conv_space_host_driver

build/%.o: $(CSRC)/%.hip $(wildcard $(CSRC)/*.hpp) ../../include/nifty_amd.h
	@mkdir -p build
	$(HIPCC) $(CXXFLAGS) -c $< -o $@

build/libnifty_amd_conv_space_asan.so: $(OBJS)
	$(HIPCC) -shared --offload-arch=$(ARCH) -fsanitize=address -fno-gpu-sanitize -o $@ $(OBJS)

build/conv_space_host_driver: conv_space_host_driver.cpp build/libnifty_amd_conv_space_asan.so
	$(HIPCC) -O1 -g -std=c++17 -I../../include -fsanitize=address -fno-omit-frame-pointer -fno-gpu-sanitize \
	  conv_space_host_driver.cpp -o $@ -Lbuild -lnifty_amd_conv_space_asan -Wl,-rpath,'$$ORIGIN'

.PHONY: all
