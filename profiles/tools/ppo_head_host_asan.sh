#!/bin/bash
# The host half of ftl_ppo_head (argument checks, workspace and segment arithmetic) under -fsanitize=address,undefined, as a stand-alone
# program: the library's two translation units with the host side instrumented, linked with ppo_head_host_asan.cpp.  Runs without a GPU.
# usage: ppo_head_host_asan.sh [output directory, default a fresh temporary one]
set -e -o pipefail
here="$(cd "$(dirname "$0")" && pwd)"
root="$here/../.."
out="${1:-$(mktemp -d)}"
san="-Xarch_host -fsanitize=address,undefined -Xarch_host -fno-sanitize-recover=undefined"
cd "$root/continiousenvironment_follower_leader_amd/csrc"
hipcc="${HIPCC:-/opt/rocm/bin/hipcc}"
clang="$(dirname "$("$hipcc" --version | sed -n 's/^InstalledDir: //p')")/bin/clang++"
# (the sanitizers instrument the host compilation only; the device code is compiled as always and never runs here)
for src in ftl_abi.hip ftl_scenario.cpp "$here/ppo_head_host_asan.cpp"; do
    "$hipcc" --offload-arch=gfx950 -O1 -g -ffp-contract=off -std=c++17 -pthread -I "$root/include" $san -c "$src" -o "$out/$(basename "$src").o" 2>>"$out/build.log" \
        || { tail -20 "$out/build.log"; exit 1; }
done
"$clang" -fsanitize=address,undefined -pthread "$out"/*.o -L"${ROCM_PATH:-/opt/rocm}/lib" -lamdhip64 -Wl,-rpath,"${ROCM_PATH:-/opt/rocm}/lib" -o "$out/ppo_head_host_asan" 2>>"$out/build.log" \
    || { tail -20 "$out/build.log"; exit 1; }
"$out/ppo_head_host_asan"
