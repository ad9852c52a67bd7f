// Host-side launcher of the structure-only kernel (structure_only.hip): StructureOnlySolver<PointDoF>::calc
// (g2o/solvers/structure_only/structure_only_solver.h:72-212) for every selected landmark in one launch.
#pragma once
#include <hip/hip_runtime.h>

namespace g2ohip {
namespace launch {

constexpr int SO_WIDTH = 8;                     // lanes per landmark (structure-only: why 8)
constexpr int SO_BLOCK = 256;                   // threads per block
constexpr int SO_LMS = SO_BLOCK / SO_WIDTH;     // landmarks per block
constexpr int SO_COUNTS = 5;                    // accepted, rejected, gradient stops, exhausted trials, fixed skipped

// one device edge group as seen from its landmark end: the landmark's estimate comes from the kernel's registers, the
// other vertex (camera, pose; none for a prior) from its state array
struct SoGroup {
  const int* vo;         // per edge: local index of the other vertex in `so` (nullptr: a unary edge)
  const double* so;      // state array of the other vertex's type
  const double* meas;    // family payload (device_types.hpp)
  const double* info;    // packed upper information
  const double* params;  // intrinsics / sensor offset record
  double rk_delta;       // robust kernel of the edge set: RobustKernel::delta
  int rk;                // G2OHIP_RK_*, 0 none
  int ue;                // uniform records: bit 0 information, bit 1 parameters (EdgeData::ue)
  int family;            // FAM_*
  int pad_;
};

struct SoCall {
  const SoGroup* groups;          // the edge groups with a landmark end
  const int* lm_ptr;              // per landmark: its range in `ent` (nlm + 1)
  const int2* ent;                // (group, edge in the group), per landmark in group order, then edge order
  const int* lm_local;            // per landmark: its index in the point state array
  const unsigned char* lm_fixed;  // per landmark: fixed (skipped, :104)
  const int* sel;                 // the selected landmarks (nullptr: 0 .. nsel - 1)
  int nsel;
  double* pts;                    // point state array (3 or 2 doubles per point), the only array written
  int num_iters, max_trials;
  long long* part;                // per block SO_COUNTS partial counts
};

inline int so_blocks(int nsel) { return (nsel + SO_LMS - 1) / SO_LMS; }
// ld: 3 (VertexSBAPointXYZ / VertexPointXYZ) or 2 (VertexPointXY). single_family: the one FAM_* every entry belongs to
// when the templated fast kernel exists for it (FAM_BA, FAM_SE2XY), else -1 (the dispatching kernel)
void structure_only(int ld, int single_family, const SoCall& c, hipStream_t s);

}  // namespace launch
}  // namespace g2ohip
