# tests/mock_gpu/uu.mk -- TEST INFRASTRUCTURE: what the uu read filter adds to the makefiles beside it.  A change that adds
# a feature leaves the existing files under tests/ as they are, so the filter (host/sources.mk: LIBSRC_UU), its stand-in
# and the one-core benchmark stand here, and tests/uu_mock_build.py builds them with `make -f uu.mk` into a directory of
# its own: the libraries of tests/mock_build.py stay what they were.  A later change that may edit the Makefile folds
# these into MOCK, LIBSRC and the rules-bench targets and deletes this file.
include GNUmakefile

UU_GPU   = la_gpu_uu_mock.o
UU_HOST  = $(LIBSRC_UU:.c=.o)

# The two libraries under names of their own: a process that has loaded mock_build.py's libla_gpu_mock.so would hand that
# one to any library that asks for the name again, and it has no la_gpu_uu_decode.
$(OUT)/libla_gpu_mock_uu.so: $(addprefix $(PLAIN)/,$(GPU_OBJ) $(LZOP_COMP) $(UU_GPU))
	$(CXX) -shared -o $@ $^ -lz $(BZ2)
$(OUT)/libla_host_mock_uu.so: $(addprefix $(PLAIN)/,$(HOST_OBJ) $(UU_HOST)) $(OUT)/libla_gpu_mock_uu.so
	$(CC) -shared -Wl,--no-undefined -o $@ $(addprefix $(PLAIN)/,$(HOST_OBJ) $(UU_HOST)) -L$(OUT) -lla_gpu_mock_uu -Wl,-rpath,'$$ORIGIN' -lpthread

# the sanitizer programs link `$^`: the filter and its stand-in join them
$(addprefix $(OUT)/,$(SAN_PROGS)): $(addprefix $(ASAN)/,$(UU_HOST) $(UU_GPU))

# at -O2, for tools/measure_uu.py's one-core baseline
$(OUT)/uu_rules_bench: uu_rules_bench.c la_gpu_uu_mock.c $(CSRC)/la_uu_dev.h ../../include/la_gpu.h
	$(CC) -O2 $(WARN) -std=gnu11 -o $@ uu_rules_bench.c la_gpu_uu_mock.c
