# Sanitizer builds of the packed ROI transfer's host code: tests/asan/roi_pack_main.cpp + ghost_amd/csrc/roi_pack.hip,
# once with AddressSanitizer + UBSan and once with ThreadSanitizer on the host pass (-Xarch_host; the device code is
# compiled as usual and never launched).  Both run on the CPU.
#   bash tools/asan_roi_pack.sh  -> build/asan/roi_pack_asan, build/asan/roi_pack_tsan, then runs them.
set -e
cd "$(dirname "$0")/.."
OUT=build/asan
mkdir -p $OUT
HIPCC=${HIPCC:-/opt/rocm/bin/hipcc}
FLAGS="-O1 -g -std=c++17 -fPIC --offload-arch=gfx950 -Ighost_amd/csrc -Iinclude -Xarch_host -fno-omit-frame-pointer"
ASAN="-Xarch_host -fsanitize=address -Xarch_host -fsanitize=undefined"
TSAN="-Xarch_host -fsanitize=thread"
build() {   # name, sanitizer flags
  $HIPCC $FLAGS $2 -c ghost_amd/csrc/roi_pack.hip -o $OUT/roi_pack_$1.o
  $HIPCC $FLAGS $2 -c tests/asan/roi_pack_main.cpp -o $OUT/roi_pack_main_$1.obj
  $HIPCC --offload-arch=gfx950 $2 $OUT/roi_pack_main_$1.obj $OUT/roi_pack_$1.o -o $OUT/roi_pack_$1
}
build asan "$ASAN" &
a=$!
build tsan "$TSAN" &
t=$!
wait $a
wait $t
ASAN_OPTIONS=detect_leaks=1:abort_on_error=0 UBSAN_OPTIONS=print_stacktrace=1:halt_on_error=1 $OUT/roi_pack_asan
TSAN_OPTIONS=halt_on_error=1 $OUT/roi_pack_tsan
