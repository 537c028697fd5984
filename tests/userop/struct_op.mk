# TEST INFRASTRUCTURE: the device ops of the derived-type tests (tests/test_gpu_struct_op.py), built in-tree for gfx950
# with the flags of tree_op.mk (git-ignored like every .so).
#   make -C tests/userop -f struct_op.mk          libstruct_op.so, libstruct_op_all.so (__graft_entry__.build() runs this)
#   make -C tests/userop -f struct_op.mk ab       the measurement variant below
# libstruct_op.so is the header as shipped.  libstruct_op_all.so takes element groups at every size that has them and
# declines the trees the register rule keeps from the vector kernel (include/chiara_user_op.hpp CHR_USER_GROUP_VEC,
# CHR_USER_TREE_WIDE_ELEMENTWISE): the shipped policy keeps groups only where they measured faster, and the tests run
# every shape through both paths.
ROCM ?= /opt/rocm
HIPCC = $(ROCM)/bin/hipcc -O3 -std=c++17 -fPIC -shared --offload-arch=gfx950 -fno-fast-math -ffp-contract=off \
	  -I../../include
HDRS = ../../include/chiara_user_op.hpp ../../include/chiara.h
all: libstruct_op.so libstruct_op_all.so
libstruct_op.so: struct_op.hip $(HDRS)
	$(HIPCC) -o $@ $<
knobs_all = -DCHR_USER_GROUP_VEC=2 -DCHR_USER_TREE_WIDE_ELEMENTWISE=0

# Measurement only (tools/userop_bench.py --struct): element groups compiled out -- every size that does not divide
# 16 element-wise, the behaviour before the groups.
knobs_grp0 = -DCHR_USER_GROUP_VEC=0
ab: libstruct_op_grp0.so
libstruct_op_%.so: struct_op.hip $(HDRS)
	$(HIPCC) $(knobs_$*) -o $@ $<
.PHONY: all ab
