# TEST ONLY: the emulation library with the partition search's counters (scan_counters.h) for tests/test_emu_scan_step.py:
#   make -C tests/emu -f scan_counters.mk   -> build/libh264e_emu_scan.so
# The same sources and flags as build/libh264e_emu.so (Makefile), with scan_counters.h included in front of emu_backend.cpp.
include Makefile
scan: build/libh264e_emu_scan.so
build/libh264e_emu_scan.so: emu_backend.cpp emu_hip.h emu_handoffs.h scan_counters.h $(SRC)/*.h build/host.o
	$(CXX) -std=c++17 -O2 -g -fPIC -DH264E_EMU -include scan_counters.h -c emu_backend.cpp -o build/emu_scan.o
	$(CXX) -shared -o $@ build/emu_scan.o build/host.o
.DEFAULT_GOAL := scan
.PHONY: scan
