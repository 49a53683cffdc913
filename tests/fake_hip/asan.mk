# The host side of the library + the fake runtime + the threaded driver (mt_drive.cpp) under the address and undefined-behaviour sanitizers: one executable, the
# sanitizer runtime linked in (no preload needed).  CPU only: make -C tests/fake_hip -f asan.mk.  The units and the pattern rules are the Makefile's.
SAN ?= -fsanitize=address,undefined -fno-omit-frame-pointer
TAG ?= asan
.DEFAULT_GOAL := mt_drive_$(TAG)
include Makefile
mt_drive_$(TAG): $(call objs,.$(TAG)) mt_drive.$(TAG).o
	$(HIPCC) $(SAN) -rdynamic -o $@ $^ -ldl -lpthread
