#!/bin/bash
# A/B builds of the library with extra -D flags on one kernel file: tools/build_variant.sh NAME FILE.hip "-DFLAG ..."  ->  c3poa_amd/lib/libc3poa_hip_NAME.so
# (the object list is the Makefile's: its `variant` target swaps FILE's object for one built with the extra flags)
set -e
make -s -j8 -C "$(dirname "$0")/../c3poa_amd/csrc" variant NAME="$1" FILE="$2" VFLAGS="$3" >/dev/null
echo built ../lib/libc3poa_hip_$1.so
