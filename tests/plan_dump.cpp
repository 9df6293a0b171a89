// The C plan of the PPS test net as JSON, on a CPU: what pps_model_create
// builds before it touches the device (pps_amd/csrc/model_plan.hpp), for
// tests/test_model_plan_host.py to compare with pps_amd.model.build_plan().
//
//   plan_dump height width strip_num bpm_dim num_groups width_per_group
//             stride_1x1 res5_stride res5_dilation fpn_on fpn_dim max_ave normalize
//
// (the PpsModelConfig integers that shape the plan, in the struct's order)
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "../pps_amd/csrc/model_plan.hpp"

namespace {

void put(const std::string& s) {  // blob names: no character needs escaping
  std::printf("\"%s\"", s.c_str());
}
template <class T> void put_ints(const std::vector<T>& v) {
  std::printf("[");
  for (size_t i = 0; i < v.size(); ++i) std::printf("%s%lld", i ? ", " : "", (long long)v[i]);
  std::printf("]");
}
void put_strings(const std::vector<std::string>& v) {
  std::printf("[");
  for (size_t i = 0; i < v.size(); ++i) {
    if (i) std::printf(", ");
    put(v[i]);
  }
  std::printf("]");
}

void put_layer(const pps::PlanLayer& L) {
  std::printf("{\"op\": ");
  put(pps::op_name(L.op));
  const std::pair<const char*, const std::string*> strs[] = {
      {"name", &L.name}, {"bn", &L.bn}, {"input", &L.input}, {"output", &L.output},
      {"residual", &L.residual}};
  for (const auto& kv : strs) {
    std::printf(", \"%s\": ", kv.first);
    put(*kv.second);
  }
  const std::pair<const char*, int> ints[] = {
      {"cin", L.cin}, {"cout", L.cout}, {"k", L.k}, {"stride", L.stride}, {"pad", L.pad},
      {"dil", L.dil}, {"relu", L.relu}, {"max_ave", L.max_ave}, {"dim", L.dim},
      {"dim_inner", L.dim_inner}};
  for (const auto& kv : ints) std::printf(", \"%s\": %d", kv.first, kv.second);
  std::printf(", \"split\": ");
  put_ints(L.split);
  std::printf(", \"prefixes\": ");
  put_strings(L.prefixes);
  std::printf("}");
}

}  // namespace

int main(int argc, char** argv) {
  if (argc != 14) {
    std::fprintf(stderr, "usage: %s <13 PpsModelConfig integers, height .. normalize>\n", argv[0]);
    return 2;
  }
  PpsModelConfig c;
  std::memset(&c, 0, sizeof(c));
  c.struct_size = (int)sizeof(c);
  int* const fields[13] = {&c.height, &c.width, &c.strip_num, &c.bpm_dim, &c.num_groups,
                           &c.width_per_group, &c.stride_1x1, &c.res5_stride, &c.res5_dilation,
                           &c.fpn_on, &c.fpn_dim, &c.max_ave, &c.normalize};
  for (int i = 0; i < 13; ++i) *fields[i] = std::atoi(argv[i + 1]);
  if (c.strip_num < 1 || c.strip_num > 10 || c.res5_stride < 1 || c.height <= 0) {
    std::fprintf(stderr, "bad config\n");  // what pps_model_create refuses before build_plan
    return 2;
  }
  const pps::Plan p = pps::build_plan(c);
  std::printf("{\"layers\": [");
  for (size_t i = 0; i < p.layers.size(); ++i) {
    std::printf(i ? ",\n  " : "\n  ");
    put_layer(p.layers[i]);
  }
  std::printf("\n],\n\"params\": {");
  bool first = true;
  for (const auto& kv : p.params) {
    std::printf(first ? "\n  " : ",\n  ");
    first = false;
    put(kv.first);
    std::printf(": ");
    put_ints(kv.second);
  }
  std::printf("\n},\n\"output\": ");
  put(p.output);
  std::printf(",\n\"feat_dim\": %d}\n", p.feat_dim);
  return 0;
}
