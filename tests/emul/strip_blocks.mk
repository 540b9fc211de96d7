# tests/emul/strip_blocks.mk -- TEST INFRASTRUCTURE ONLY: the strip class in blocks on the wave emulator, a library of
# its own beside libdcp_emul.so (make -f strip_blocks.mk).
HERE := $(dir $(abspath $(lastword $(MAKEFILE_LIST))))
CSRC := $(HERE)../../deciphon_amd/csrc
HDRS := $(HERE)lane_ops_emul.h $(HERE)block_walk.h $(CSRC)/viterbi_body.h $(CSRC)/traceback.h $(CSRC)/row_replay.h $(CSRC)/dcp_types.h $(CSRC)/dcp_states.h
CXXFLAGS := -std=c++17 -O2 -fPIC -ffp-contract=off -Wall -Wno-unknown-pragmas -Wno-maybe-uninitialized

all: $(HERE)libdcp_emul_strip_blocks.so

$(HERE)libdcp_emul_strip_blocks.so: $(HERE)emul_strip_blocks.cpp $(HDRS)
	g++ $(CXXFLAGS) -shared -o $@ $<

clean:
	rm -f $(HERE)libdcp_emul_strip_blocks.so
.PHONY: all clean
