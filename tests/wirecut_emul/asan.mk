# CPU-only sanitizer build of the cut harness (make -C tests/wirecut_emul asan).  Not shipped to the GPU box.
HIPCC ?= /opt/rocm/bin/hipcc
CSRC := ../../aes-gcm-128-192-256-bits_amd/csrc
SAN := -fsanitize=address,undefined
emul_asan: emul.cpp $(wildcard $(CSRC)/*.h) ../../include/aesgcm.h
	$(HIPCC) -O1 -g -std=c++17 --offload-arch=gfx950 --cuda-host-only -Wall -Wno-unused-function -Wno-unused-value $(SAN) -fno-omit-frame-pointer -o $@ emul.cpp
