// The host half of csrc/vit_snapshot.hip (argument validation in front of the launch) as a stand-alone program for the host sanitizers.
// Nothing here launches a kernel or needs a device: every call returns before hipLaunchKernelGGL.
//   cd styl3r_amd/csrc && hipcc --offload-arch=gfx950 -O1 -g -std=c++17 -Xarch_host -fsanitize=address,undefined -I../../include \
//       vit_snapshot.hip ../../tools/snapshot_host_check.cpp -o /tmp/snapshot_host_check && /tmp/snapshot_host_check
#include <hip/hip_runtime.h>
#include <cstdio>
#include <cstdlib>

#include "vit_ops.h"

namespace vit {
thread_local hipError_t g_last_hip_error = hipSuccess;       // (vit_api.hip owns it in the library)
size_t snapshot_chunk_bytes();
int snapshot_pack(const VitSnapChunk *chunks, int n_chunks, void *staging, VitSnapPartial *partials, hipStream_t stream);
}  // namespace vit

#define EXPECT(cond) do { if (!(cond)) { std::fprintf(stderr, "FAILED: %s (line %d)\n", #cond, __LINE__); return 1; } } while (0)

int main()
{
    EXPECT(sizeof(VitSnapChunk) == 24 && sizeof(VitSnapPartial) == 24);
    const size_t chunk = vit::snapshot_chunk_bytes();
    EXPECT(chunk >= 4096 && chunk % 64 == 0);
    alignas(64) static unsigned char staging[256];
    static VitSnapPartial partials[2];
    static VitSnapChunk table[2] = {{staging, 0, 16, VIT_SNAP_VEC16}, {staging + 64, 64, 7, 0}};
    EXPECT(vit::snapshot_pack(nullptr, 0, nullptr, nullptr, nullptr) == VIT_OK);          // nothing to do: no launch
    EXPECT(vit::snapshot_pack(nullptr, 2, staging, partials, nullptr) == VIT_EINVAL);
    EXPECT(vit::snapshot_pack(table, -1, staging, partials, nullptr) == VIT_EINVAL);
    EXPECT(vit::snapshot_pack(table, 2, nullptr, partials, nullptr) == VIT_EINVAL);
    EXPECT(vit::snapshot_pack(table, 2, staging, nullptr, nullptr) == VIT_EINVAL);
    EXPECT(vit::snapshot_pack(table, 2, staging + 32, partials, nullptr) == VIT_EINVAL);  // staging: 64-byte aligned
    EXPECT(vit::snapshot_pack(table, 2, staging, reinterpret_cast<VitSnapPartial *>(reinterpret_cast<unsigned char *>(partials) + 4), nullptr) == VIT_EINVAL);
    std::puts("snapshot_host_check OK");
    return 0;
}
