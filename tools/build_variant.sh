#!/bin/bash
# Build a variant of the experiments library with extra compile flags: tools/build_variant.sh <name> [-DFLAG=V ...]
# -> infinite-video_amd/libinfv_ltm_v_<name>.so (git-ignored; select it with INFV_LTM_LIBRARY=<path>).  Same-box A/B: tools/ab_libs.sh.
set -e
name=$1; shift
cd "$(dirname "$0")/.."
/opt/rocm/bin/hipcc -O3 --offload-arch=gfx950 -std=c++17 -fPIC -shared -I include -DINFV_EXPERIMENTS "$@" -o infinite-video_amd/libinfv_ltm_v_$name.so infinite-video_amd/csrc/*.hip
echo "built infinite-video_amd/libinfv_ltm_v_$name.so"
