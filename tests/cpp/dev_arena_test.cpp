// Drives the planner of visual-slam_amd/csrc/dev_arena.h (as plain C++, no HIP) with a scripted list of typed requests
// and prints what it assigned; tests/test_dev_arena_cpu.py holds the expected values.
//
// stdin:  one request per line: type count     (type c = char, i = int, d = double, r = a 12-byte record)
// stdout: one line per request: offset of the bound pointer from the base
//         last line: total n_requests
#include <cstdio>
#include <vector>

#include "dev_arena.h"

struct Rec12 { int v[3]; };

int main() {
  // the pointers the plan assigns: one of the four is used per request (addresses stay put: sized before the first add)
  const size_t cap = 64;
  std::vector<char*> pc(cap, nullptr);
  std::vector<int*> pi(cap, nullptr);
  std::vector<double*> pd(cap, nullptr);
  std::vector<Rec12*> pr(cap, nullptr);
  std::vector<char> type;
  ArenaPlan plan;
  char t;
  unsigned long long count;
  while (scanf(" %c %llu", &t, &count) == 2) {
    const size_t k = type.size();
    if (k >= cap) return 2;
    if (t == 'c') plan.add(pc[k], (size_t)count);
    else if (t == 'i') plan.add(pi[k], (size_t)count);
    else if (t == 'd') plan.add(pd[k], (size_t)count);
    else if (t == 'r') plan.add(pr[k], (size_t)count);
    else return 3;
    type.push_back(t);
  }
  std::vector<char> block(plan.total() + 1);
  char* base = block.data();
  plan.bind(base);
  for (size_t k = 0; k < type.size(); k++) {
    const char* p = type[k] == 'c' ? pc[k] : type[k] == 'i' ? (const char*)pi[k] : type[k] == 'd' ? (const char*)pd[k] : (const char*)pr[k];
    printf("%lld\n", p ? (long long)(p - base) : -1LL);
  }
  printf("total %zu %zu\n", plan.total(), type.size());
  return 0;
}
