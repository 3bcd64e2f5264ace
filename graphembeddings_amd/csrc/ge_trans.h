// ge_trans.h -- "which translation model, which tables": what ge_capi.hip validates once per call and every
// translation launcher takes (host side only), the tables as the sweep kernels take them, and the one dispatcher from
// the runtime (model, l1) to the kernels' <MODEL, L1>.
#pragma once
#include <stdint.h>

#include <type_traits>

#include "../../include/ge_hip.h"

namespace ge {

constexpr int kTransE = GE_TRANSX_TRANSE, kTransH = GE_TRANSX_TRANSH, kTransD = GE_TRANSX_TRANSD;
constexpr int kTransR = 3;               // the library's own code for TransR (not an ABI value)

// One call's model: the tables under their ABI names (null where the model has none).  TransE / TransH / TransD:
// dE = dq = d.  TransR: dE = dim_e, dq = dim_r.  The size functions fill the shape alone.
struct TransModel {
  int model, l1;
  const float* ent;            // [E, dE]
  const float* rel;            // [R, dq]
  const float* normal;         // TransH [R, d]
  const float* ent_transfer;   // TransD [E, d]
  const float* rel_transfer;   // TransD [R, d]
  const float* rel_matrix;     // TransR [R, dq * dE]
  int64_t E, R;
  int dE, dq;                  // entity width; width of a relation row, of a query and of the distance
};

// The tables of one call as the kernels read them (trans_prepare, ge_trans_dev.h, fills it).  The rank and top-k
// kernels take it by value: the field order is their argument layout.
struct TransTables {
  const float* ent;     // [E, dE]
  const float* rel;     // [R, dq]
  const float* aux;     // TransH: n^ [R, d] (workspace);  TransD: rel_transfer [R, d];  TransR: rel_matrix [R, dq*dE]
  const float* ent2;    // TransD: ent_transfer [E, d]
  const float* A;       // TransD: A_c = e_c . e_p,c [E] (workspace), where the sweep asks for it
  int64_t E, R;
  int dE, dq;           // entity width; width of q and of the distance (d for TransX, dim_r for TransR)
};

// f(std::integral_constant<int, MODEL>, std::bool_constant<L1>) for m's model and norm.
template <class F>
auto dispatch_trans(const TransModel& m, F f) {
  auto norm = [&](auto model) { return m.l1 ? f(model, std::true_type{}) : f(model, std::false_type{}); };
  switch (m.model) {
    case kTransE: return norm(std::integral_constant<int, kTransE>{});
    case kTransH: return norm(std::integral_constant<int, kTransH>{});
    case kTransD: return norm(std::integral_constant<int, kTransD>{});
    default: return norm(std::integral_constant<int, kTransR>{});
  }
}

}  // namespace ge
