# TEST INFRASTRUCTURE: the device op of the one-pass user-op tree tests (tests/test_gpu_user_tree.py), built in-tree
# for gfx950 with the flags of this directory's Makefile (git-ignored like every .so).
#   make -C tests/userop -f tree_op.mk          libhalfadd_tree_op.so (__graft_entry__.build() runs this)
#   make -C tests/userop -f tree_op.mk ab       the measurement variants below
ROCM ?= /opt/rocm
HIPCC = $(ROCM)/bin/hipcc -O3 -std=c++17 -fPIC -shared --offload-arch=gfx950 -fno-fast-math -ffp-contract=off \
	  -I../../include
HDRS = ../../include/chiara_user_op.hpp ../../include/chiara.h
libhalfadd_tree_op.so: halfadd_tree_op.hip $(HDRS)
	$(HIPCC) -o $@ $<

# Measurement only (tools/userop_bench.py --ab): the tree op built with the one-pass kernel's policy knobs set the
# other way -- non-temporal accesses off, XCD runs off or 512 KiB -- against the shipped NT = 1, 256 KiB.
AB = nt0_xcd0 nt1_xcd0 nt0_xcd256 nt1_xcd512
knobs_nt0_xcd0 = -DCHR_USER_TREE_NT=0 -DCHR_USER_TREE_XCD_RUN_KIB=0
knobs_nt1_xcd0 = -DCHR_USER_TREE_NT=1 -DCHR_USER_TREE_XCD_RUN_KIB=0
knobs_nt0_xcd256 = -DCHR_USER_TREE_NT=0 -DCHR_USER_TREE_XCD_RUN_KIB=256
knobs_nt1_xcd512 = -DCHR_USER_TREE_NT=1 -DCHR_USER_TREE_XCD_RUN_KIB=512
ab: $(AB:%=libhalfadd_tree_op_%.so)
libhalfadd_tree_op_%.so: halfadd_tree_op.hip $(HDRS)
	$(HIPCC) $(knobs_$*) -o $@ $<
.PHONY: ab
