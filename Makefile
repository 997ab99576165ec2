# Builds the gfx950 HIP library kelpie_amd/libkelpie_hip.so (C ABI: include/kelpie_hip.h)
HIPCC ?= /opt/rocm/bin/hipcc
ARCH ?= gfx950
SRC := $(wildcard kelpie_amd/csrc/*.hip)
CPP := $(wildcard kelpie_amd/csrc/*.cpp)
OBJ := $(patsubst kelpie_amd/csrc/%.hip,build/%.o,$(SRC)) $(patsubst kelpie_amd/csrc/%.cpp,build/%.cpp.o,$(CPP))
CXX ?= g++
FLAGS := --offload-arch=$(ARCH) -O3 -std=c++17 -fPIC -ffp-contract=off -Wall -Wno-unused-function \
         -Wno-unused-result -Iinclude -Xarch_host -mavx2
LIB := kelpie_amd/libkelpie_hip.so

all: $(LIB)

build/%.o: kelpie_amd/csrc/%.hip kelpie_amd/csrc/kp_common.hpp kelpie_amd/csrc/kp_attn.hpp kelpie_amd/csrc/kp_attn_plan.hpp kelpie_amd/csrc/kp_attn3.hpp kelpie_amd/csrc/kp_cv_fused.hpp kelpie_amd/csrc/kp_posttrain.hpp kelpie_amd/csrc/kp_batch_check.hpp kelpie_amd/csrc/kp_probe_check.hpp kelpie_amd/csrc/kp_trace_check.hpp kelpie_amd/csrc/kp_marks_check.hpp kelpie_amd/csrc/kp_cx_plan.hpp kelpie_amd/csrc/kp_cv_plan.hpp include/kelpie_hip.h
	@mkdir -p build
	$(HIPCC) $(FLAGS) -c $< -o $@

# host-only C++ (prefilter graphs)
build/%.cpp.o: kelpie_amd/csrc/%.cpp include/kelpie_hip.h
	@mkdir -p build
	$(CXX) -O3 -std=c++17 -fPIC -Wall -mavx2 -pthread -Iinclude $(if $(findstring kp_rng,$<),-ffp-contract=off -mfma) -c $< -o $@

$(LIB): $(OBJ)
	$(HIPCC) --offload-arch=$(ARCH) -shared -fPIC -pthread -o $@ $(OBJ)

resources: $(SRC)
	@mkdir -p build
	for f in $(SRC); do $(HIPCC) $(FLAGS) -c $$f -o /dev/null -Rpass-analysis=kernel-resource-usage 2>&1 | grep -E "Function Name|VGPRs:|AGPRs|Spill|Occupancy|LDS" ; done

# diagnostic build: kp_attn phase timestamps (s_memtime), kelpie_amd/libkelpie_hip_stamps.so
stamps:
	@mkdir -p build/stamps
	for f in $(SRC); do $(HIPCC) $(FLAGS) -DKP_ATTN_STAMPS -DKP_TE_STAMPS -c $$f -o build/stamps/$$(basename $$f .hip).o || exit 1; done
	$(HIPCC) --offload-arch=$(ARCH) -shared -fPIC -pthread -o kelpie_amd/libkelpie_hip_stamps.so build/stamps/*.o $(patsubst kelpie_amd/csrc/%.cpp,build/%.cpp.o,$(CPP))

# timing-only diagnostic variants (wrong results), never the product library:
#   make diag DIAG="nos:-DKP_DIAG_NO_S noo:-DKP_DIAG_NO_O nodma:-DKP_ATTN_NODMA"  (commas: several defines)
# builds variants/lib_<name>.so, loaded by tools/attn_phase_ab.sh through KELPIE_HIP_LIB
DIAG ?= nos:-DKP_DIAG_NO_S noo:-DKP_DIAG_NO_O nodma:-DKP_ATTN_NODMA
diag: $(patsubst kelpie_amd/csrc/%.cpp,build/%.cpp.o,$(CPP))
	@mkdir -p variants
	for v in $(DIAG); do n=$${v%%:*}; d=$$(echo $${v#*:} | tr , ' '); mkdir -p build/diag_$$n; \
	  for f in $(SRC); do $(HIPCC) $(FLAGS) -DKP_DIAGNOSTIC_BUILD $$d -c $$f -o build/diag_$$n/$$(basename $$f .hip).o || exit 1; done; \
	  $(HIPCC) --offload-arch=$(ARCH) -shared -fPIC -pthread -o variants/lib_$$n.so build/diag_$$n/*.o $^ || exit 1; done

clean:
	rm -rf build $(LIB)

.PHONY: all clean resources stamps diag

# host sanitizer builds of the library's host C++ (kp_rng.cpp worker pool / arenas,
# kp_graph.cpp) linked into tests/native/host_san_driver.cpp; run by
# tests/test_host_sanitizers.py (CPU suite), or by hand: make asan tsan
SAN_SRC := kelpie_amd/csrc/kp_rng.cpp kelpie_amd/csrc/kp_graph.cpp kelpie_amd/csrc/kp_sched.cpp tests/native/host_san_driver.cpp
SAN_FLAGS := -O1 -g -std=c++17 -fno-omit-frame-pointer -mavx2 -mfma -ffp-contract=off -pthread -Iinclude
asan: build/san/host_asan
tsan: build/san/host_tsan
build/san/host_asan: $(SAN_SRC) include/kelpie_hip.h
	@mkdir -p build/san
	$(CXX) $(SAN_FLAGS) -fsanitize=address,undefined -fno-sanitize-recover=undefined $(SAN_SRC) -o $@
build/san/host_tsan: $(SAN_SRC) include/kelpie_hip.h
	@mkdir -p build/san
	$(CXX) $(SAN_FLAGS) -fsanitize=thread $(SAN_SRC) -o $@

# the post-training batch check (kp_batch_check.hpp, no HIP) alone in
# tests/native/batch_check_driver.cpp; run by tests/test_batch_check.py (CPU suite)
batch_asan: build/san/batch_check_asan
build/san/batch_check_asan: tests/native/batch_check_driver.cpp kelpie_amd/csrc/kp_batch_check.hpp include/kelpie_hip.h
	@mkdir -p build/san
	$(CXX) -O1 -g -std=c++17 -fno-omit-frame-pointer -fsanitize=address,undefined -fno-sanitize-recover=undefined $< -o $@

# the attention planners (kp_attn_plan.hpp, no HIP) alone in tests/native/attn_plan_driver.cpp,
# plain and under the host sanitizers; run by tests/test_attn_plan.py (CPU suite)
attn_plan: build/san/attn_plan
attn_plan_asan: build/san/attn_plan_asan
build/san/attn_plan: tests/native/attn_plan_driver.cpp kelpie_amd/csrc/kp_attn_plan.hpp
	@mkdir -p build/san
	$(CXX) -O2 -std=c++17 -Wall $< -o $@
build/san/attn_plan_asan: tests/native/attn_plan_driver.cpp kelpie_amd/csrc/kp_attn_plan.hpp
	@mkdir -p build/san
	$(CXX) -O1 -g -std=c++17 -Wall -fno-omit-frame-pointer -fsanitize=address,undefined -fno-sanitize-recover=undefined $< -o $@

# the post-training step planners (kp_cx_plan.hpp, kp_cv_plan.hpp, no HIP) alone in
# tests/native/step_plan_driver.cpp, plain and under the host sanitizers; run by
# tests/test_step_plan.py (CPU suite)
STEP_PLAN_DEP := tests/native/step_plan_driver.cpp kelpie_amd/csrc/kp_cx_plan.hpp kelpie_amd/csrc/kp_cv_plan.hpp include/kelpie_hip.h
step_plan: build/san/step_plan
step_plan_asan: build/san/step_plan_asan
build/san/step_plan: $(STEP_PLAN_DEP)
	@mkdir -p build/san
	$(CXX) -O2 -std=c++17 -Wall $< -o $@
build/san/step_plan_asan: $(STEP_PLAN_DEP)
	@mkdir -p build/san
	$(CXX) -O1 -g -std=c++17 -Wall -fno-omit-frame-pointer -fsanitize=address,undefined -fno-sanitize-recover=undefined $< -o $@

# the probes' check and chunking (kp_probe_check.hpp, no HIP) alone in
# tests/native/probe_check_driver.cpp, plain and under the host sanitizers; run by
# tests/test_probe_check.py (CPU suite)
PROBE_CHECK_DEP := tests/native/probe_check_driver.cpp kelpie_amd/csrc/kp_probe_check.hpp include/kelpie_hip.h
probe_check: build/san/probe_check
probe_check_asan: build/san/probe_check_asan
build/san/probe_check: $(PROBE_CHECK_DEP)
	@mkdir -p build/san
	$(CXX) -O2 -std=c++17 -Wall $< -o $@
build/san/probe_check_asan: $(PROBE_CHECK_DEP)
	@mkdir -p build/san
	$(CXX) -O1 -g -std=c++17 -Wall -fno-omit-frame-pointer -fsanitize=address,undefined -fno-sanitize-recover=undefined $< -o $@

# the trace's step counts and check (kp_trace_check.hpp, no HIP) alone in
# tests/native/trace_check_driver.cpp, plain and under the host sanitizers; run by
# tests/test_trace_check.py (CPU suite)
TRACE_CHECK_DEP := tests/native/trace_check_driver.cpp kelpie_amd/csrc/kp_trace_check.hpp include/kelpie_hip.h
trace_check: build/san/trace_check
trace_check_asan: build/san/trace_check_asan
build/san/trace_check: $(TRACE_CHECK_DEP)
	@mkdir -p build/san
	$(CXX) -O2 -std=c++17 -Wall $< -o $@
build/san/trace_check_asan: $(TRACE_CHECK_DEP)
	@mkdir -p build/san
	$(CXX) -O1 -g -std=c++17 -Wall -fno-omit-frame-pointer -fsanitize=address,undefined -fno-sanitize-recover=undefined $< -o $@

# the epoch marks' check and plan (kp_marks_check.hpp, no HIP) alone in
# tests/native/marks_check_driver.cpp, plain and under the host sanitizers; run by
# tests/test_marks_check.py (CPU suite)
MARKS_CHECK_DEP := tests/native/marks_check_driver.cpp kelpie_amd/csrc/kp_marks_check.hpp kelpie_amd/csrc/kp_trace_check.hpp include/kelpie_hip.h
marks_check: build/san/marks_check
marks_check_asan: build/san/marks_check_asan
build/san/marks_check: $(MARKS_CHECK_DEP)
	@mkdir -p build/san
	$(CXX) -O2 -std=c++17 -Wall $< -o $@
build/san/marks_check_asan: $(MARKS_CHECK_DEP)
	@mkdir -p build/san
	$(CXX) -O1 -g -std=c++17 -Wall -fno-omit-frame-pointer -fsanitize=address,undefined -fno-sanitize-recover=undefined $< -o $@

.PHONY: asan tsan batch_asan attn_plan attn_plan_asan step_plan step_plan_asan probe_check probe_check_asan \
        trace_check trace_check_asan marks_check marks_check_asan
