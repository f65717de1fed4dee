// fl_knobs.cpp -- the table behind fl_knobs.h and its C-ABI (fl_tuning_set / fl_tuning_get).  Plain C++: no HIP in here.
#include <cctype>
#include <cstdlib>
#include <cstring>
#include <mutex>
#include <string>

#include "../../include/fluca_hip.h"
#include "fl_knobs.h"

namespace fl {
namespace {
struct KnobEntry {
  const char      *name;
  int              dflt;
  std::atomic<int> v;
};
KnobEntry g_knobs[K_COUNT + 1] = {
#define X(n, d) {#n, (d), {(d)}},
    FL_PUBLIC_KNOBS(X)
#undef X
        {nullptr, 0, {0}}};
// the one place where the library reads its environment: FLUCA_<NAME> gives a knob its initial value
void knob_table_init()
{
  static std::once_flag once;
  std::call_once(once, []() {
    for (int k = 0; k < K_COUNT; ++k) {
      std::string env = "FLUCA_";
      for (const char *c = g_knobs[k].name; *c; ++c) env.push_back((char)std::toupper((unsigned char)*c));
      if (const char *e = std::getenv(env.c_str())) g_knobs[k].v.store(std::atoi(e), std::memory_order_relaxed);
    }
  });
}
}  // namespace
int knob(Knob k)
{
  knob_table_init();
  return g_knobs[k].v.load(std::memory_order_relaxed);
}
void knob_set(Knob k, int v)
{
  knob_table_init();
  g_knobs[k].v.store(v, std::memory_order_relaxed);
}
int knob_find(const char *name)
{
  for (int k = 0; k < K_COUNT; ++k)
    if (std::strcmp(g_knobs[k].name, name) == 0) return k;
  return -1;
}
const char *knob_name(int k) { return k >= 0 && k < K_COUNT ? g_knobs[k].name : nullptr; }
}  // namespace fl

using namespace fl;

extern "C" int fl_tuning_set(const char *name, int value)
{
  if (!name) return FL_ERR_ARG_NULL;
  const int k = knob_find(name);
  if (k < 0) return FL_ERR_ARG_WRONG;
  knob_set((Knob)k, value);
  return FL_SUCCESS;
}
extern "C" int fl_tuning_get(const char *name, int *value)
{
  if (!name || !value) return FL_ERR_ARG_NULL;
  const int k = knob_find(name);
  if (k < 0) return FL_ERR_ARG_WRONG;
  *value = knob((Knob)k);
  return FL_SUCCESS;
}
