// The conv planner as a host program, for AddressSanitizer / UBSan (tools/README.md has the build line): plans for the descriptions of
// tests/test_plan_decomposition.py's sweep, NUM_CUS walked over 8 .. 320, 512 and 4096 under every option set below, every layer's kernel name and
// launch parameters read back.  Links common.cpp, cnn_net.hip and cnn_plan.hip only -- no kernel, no device: it supplies the CU count itself.
#include <cstdio>
#include <vector>

#include "msi_hip.h"

namespace msi_cnn { int device_cu_count() { return 256; } }   // (cnn.hip's asks the device; DEFAULT_CUS where there is none)

int main() {
  const msi_net_desc descs[] = {   // batch, height, width, in_channels, num_outputs, ngf, coord_net, dtype
      {1, 320, 640, 192, 64, 64, 1, MSI_DTYPE_F32},   {1, 320, 640, 192, 64, 64, 0, MSI_DTYPE_F32}, {16, 320, 640, 384, 128, 64, 1, MSI_DTYPE_BF16},
      {32, 640, 1280, 192, 64, 64, 1, MSI_DTYPE_F32}, {64, 256, 256, 192, 64, 64, 1, MSI_DTYPE_F32}, {1, 64, 128, 96, 32, 64, 1, MSI_DTYPE_F32},
      {1, 32, 384, 96, 32, 32, 1, MSI_DTYPE_F32},     {3, 64, 128, 96, 32, 64, 0, MSI_DTYPE_F32},   {2, 32, 128, 64, 16, 64, 0, MSI_DTYPE_BF16},
      {1, 32, 128, 96, 32, 64, 0, MSI_DTYPE_F32}};
  const int ALL = 0x3ffff, EVEN = 0x15555, ODD = 0x2aaaa;   // the 18-bit per-layer masks
  struct Opt { int key, value, key2, value2; };   // (key2 < 0: one option)
  const Opt sets[] = {{-1, 0, -1, 0}, {MSI_NET_OPT_X3_TILE8, ALL | (1 << 30), -1, 0}, {MSI_NET_OPT_X3_TILE8, EVEN | (1 << 30), -1, 0}, {MSI_NET_OPT_X3_TILE8, 0, -1, 0},
                      {MSI_NET_OPT_TAILSPLIT, 0, -1, 0}, {MSI_NET_OPT_TAILSPLIT, 2, -1, 0}, {MSI_NET_OPT_UNIFORM_SPLIT, 2, -1, 0}, {MSI_NET_OPT_UNIFORM_SPLIT, 3, -1, 0},
                      {MSI_NET_OPT_UNIFORM_SPLIT, 4, -1, 0}, {MSI_NET_OPT_SPLIT_OVERHEAD, 4, -1, 0}, {MSI_NET_OPT_HALO, 0, -1, 0}, {MSI_NET_OPT_HALO, 7, -1, 0},
                      {MSI_NET_OPT_F32_SPLIT3, 0, MSI_NET_OPT_HALO, 7}, {MSI_NET_OPT_F32_SPLIT3, EVEN, MSI_NET_OPT_HALO, 7}, {MSI_NET_OPT_F32_SPLIT3, ODD, -1, 0},
                      {MSI_NET_OPT_F32_SPLIT_F16, ALL, -1, 0}, {MSI_NET_OPT_F32_SPLIT_F16, ODD, MSI_NET_OPT_X3_TILE8, ALL | (1 << 30)}, {MSI_NET_OPT_X3_ROWPAR, 0, -1, 0},
                      {MSI_NET_OPT_X3_ROWPAR, EVEN, -1, 0}, {MSI_NET_OPT_HALO_SKIP, ALL, -1, 0}, {MSI_NET_OPT_HALO_SKIP, ODD | (1 << 20), -1, 0}, {MSI_NET_OPT_BIGTILE, 0, -1, 0},
                      {MSI_NET_OPT_BIGTILE, 2, -1, 0}, {MSI_NET_OPT_BF16_STAGE_RAW, 3, MSI_NET_OPT_BF16_WAVES, 4}, {MSI_NET_OPT_FIXUP_KERNEL, 1, MSI_NET_OPT_HEAD_FUSE_LN, 0}};
  std::vector<int> cus;
  for (int c = 8; c <= 320; ++c) cus.push_back(c);
  cus.push_back(512);
  cus.push_back(4096);
  long plans = 0, refused = 0;
  unsigned long long sum = 0;
  for (const msi_net_desc &d : descs)
    for (const Opt &o : sets) {
      msi_net_plan *pl = nullptr;
      if (msi_net_plan_create(&d, &pl) != MSI_OK) { fprintf(stderr, "plan_create: %s\n", msi_last_error_string()); return 1; }
      if (o.key >= 0 && msi_net_plan_set_option(pl, o.key, o.value) != MSI_OK) ++refused;
      if (o.key2 >= 0 && msi_net_plan_set_option(pl, o.key2, o.value2) != MSI_OK) ++refused;
      for (int c : cus) {
        if (msi_net_plan_set_option(pl, MSI_NET_OPT_NUM_CUS, c) != MSI_OK) { ++refused; continue; }   // (a refusal is an answer, not a finding: the plan stays usable)
        ++plans;
        for (int li = 0; li < MSI_NET_NUM_LAYERS; ++li) {
          char name[96];
          int32_t nblocks = 0, nsplit = 0;
          size_t need = 0;
          if (msi_net_plan_layer_kernel(pl, li, name, sizeof(name), &nblocks, &nsplit) != MSI_OK || msi_net_plan_layer_params(pl, li, nullptr, 0, &need) != MSI_OK) {
            fprintf(stderr, "layer %d: %s\n", li, msi_last_error_string());
            return 1;
          }
          std::vector<unsigned char> bytes(need);   // (exact size: an overrun of the copy is a report)
          if (msi_net_plan_layer_params(pl, li, bytes.data(), bytes.size(), nullptr) != MSI_OK) return 1;
          for (unsigned char b : bytes) sum = sum * 1099511628211ull + b;
          for (const char *s = name; *s; ++s) sum = sum * 1099511628211ull + (unsigned char)*s;
          sum += (unsigned long long)nblocks * 31 + (unsigned long long)nsplit;
          if (msi_net_plan_layer_is_normalized(pl, li) < 0 && li < MSI_NET_NUM_LAYERS - 1) return 1;
        }
        if (msi_net_plan_workspace_bytes(pl) == 0) return 1;
      }
      msi_net_plan_destroy(pl);
    }
  printf("%ld plans, %ld option values refused, checksum %016llx\n", plans, refused, sum);
  return 0;
}
