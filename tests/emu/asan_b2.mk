# qpx_backward2 (the second-order pass of the backward) under AddressSanitizer + UBSan: a driver of its own,
# asan_b2_driver.cpp, a stand-alone program over the host-thread emulation -- nothing is loaded into python under a sanitizer.
#     make -C tests/emu -f asan_b2.mk          (the driver takes ~11 min to compile, its six runs a few seconds)
# Beside Makefile, whose variables and dependency list it takes over (include), so that the two cannot drift apart: seven tile
# rows, one tile row with equalities, the 16x16 grid (knob 256), QPX_F32_WIDE, the chain-wave form at four tile rows, the
# one-wave form (knob 3072).  LDS is a heap block of exactly the size the launcher asks for (QPX_EMU_LDS_SLACK=0) and every
# array has exactly the size the C ABI documents: an index one element out of range is a reported overflow.
.DEFAULT_GOAL := asan_b2
include Makefile

$(OUT)/asan_b2_driver: asan_b2_driver.cpp $(DEPS)
	@mkdir -p $(OUT)
	$(CXX) $(CXXFLAGS) -DQPX_EMU_PTHREADS -DQPX_EMU_LDS_SLACK=0 -fsanitize=address,undefined -fno-sanitize-recover=undefined -I. -I$(CSRC) -o $@ asan_b2_driver.cpp qpx_emu.cpp

asan_b2: $(OUT)/asan_b2_driver
	@for a in "1 100 100 0" "1 12 9 3" "1 12 9 3 256" "2 12 9 3 0 wide" "1 40 52 5" "1 30 64 0 3072"; do \
		echo "asan_b2_driver $$a"; ./$(OUT)/asan_b2_driver $$a > $(OUT)/asan_b2.log 2>&1 || { tail -40 $(OUT)/asan_b2.log; exit 1; }; \
	done; echo "asan_b2: clean"
