// Host: same_source (csrc/ge_step_id.h) holds for equal identities and fails when any single field of the source
// differs; the two fields that say where in the sequence a call starts are not part of it.  The field counts are
// asserted at compile time, so a field added to a descriptor without a line here (and a comparison there) does not build.
#include <stdio.h>

#include <utility>

#include "ge_step_id.h"

using namespace ge;

// number of fields of an aggregate: the longest brace list it takes
struct Any { template <class T> operator T() const; };
template <class T, class... A> constexpr auto takes(int) -> decltype(T{std::declval<A>()...}, true) { return true; }
template <class T, class... A> constexpr bool takes(...) { return false; }
template <class T, class... A> constexpr int fields() {
  if constexpr (takes<T, A..., Any>(0)) return fields<T, A..., Any>();
  else return (int)sizeof...(A);
}

struct Field { const char* name; bool in_source; void (*change)(StepIdentity&); };

static int32_t other_i32[4];
static int64_t other_i64[4];
static char other_ws[4];

static const Field kFields[] = {
    {"seq.triples", true, [](StepIdentity& i) { i.seq.triples = other_i32; }},
    {"seq.T", true, [](StepIdentity& i) { i.seq.T += 1; }},
    {"seq.first_row", false, [](StepIdentity& i) { i.seq.first_row += 8; }},
    {"seq.B", true, [](StepIdentity& i) { i.seq.B += 1; }},
    {"seq.global_step0", false, [](StepIdentity& i) { i.seq.global_step0 += 3; }},
    {"ts.id_to_type", true, [](StepIdentity& i) { i.ts.id_to_type = other_i32 + 1; }},
    {"ts.N", true, [](StepIdentity& i) { i.ts.N += 1; }},
    {"ts.type_offsets", true, [](StepIdentity& i) { i.ts.type_offsets = other_i64; }},
    {"ts.n_types", true, [](StepIdentity& i) { i.ts.n_types += 1; }},
    {"ts.type_ids", true, [](StepIdentity& i) { i.ts.type_ids = other_i32 + 2; }},
    {"ts.seed", true, [](StepIdentity& i) { i.ts.seed ^= 1ull << 40; }},
    {"ts.padded_size", true, [](StepIdentity& i) { i.ts.padded_size += 1; }},
    {"ts.mode", true, [](StepIdentity& i) { i.ts.mode += 1; }},
    {"d", true, [](StepIdentity& i) { i.d += 2; }},
    {"direct", true, [](StepIdentity& i) { i.direct ^= 1; }},
    {"negs", true, [](StepIdentity& i) { i.negs += 1; }},
    {"workspace", true, [](StepIdentity& i) { i.workspace = other_ws; }},
};

static_assert(fields<StepSeq>() == 5 && fields<TypeSampler>() == 8 && fields<StepIdentity>() == 6,
              "a descriptor of ge_step_id.h changed: list the field in kFields and compare it in same_source");
static_assert(sizeof(kFields) / sizeof(kFields[0]) == 5 + 8 + 4, "one line per field");

int main() {
  static int32_t tri[3], types[3];
  static int64_t offs[3];
  static char ws[4];
  const StepIdentity a{{tri, 40, 0, 8, 0}, {types, 96, offs, 2, types + 1, 7, 16, 0}, 8, 1, 0, ws};
  int bad = 0;
  StepIdentity same = a;
  if (!same_source(a, same) || !same_source(same, a)) { printf("equal identities differ\n"); ++bad; }
  for (const Field& f : kFields) {
    StepIdentity b = a;
    f.change(b);
    if (same_source(a, b) == f.in_source || same_source(b, a) == f.in_source) {
      printf("%s: same_source is %s\n", f.name, f.in_source ? "true although the field differs" : "false for a position field");
      ++bad;
    }
  }
  printf("%d fields, %d wrong\n", (int)(sizeof(kFields) / sizeof(kFields[0])), bad);
  return bad ? 1 : 0;
}
