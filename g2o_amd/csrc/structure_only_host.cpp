// Engine side of the structure-only pre-pass (structure_only_solver.h:60-229): the per-landmark edge lists, the call
// and the cache invalidation after it. The kernel is in structure_only.hip.
#include <algorithm>
#include <cstring>
#include <limits>
#include <numeric>

#include "engine.hpp"

namespace g2ohip {

// PointDoF of the algorithm name (structure_only.cpp:64-65 registers structure_only_2 and structure_only_3), 0: another
// algorithm
static int so_name_dim(const std::string& algorithm) {
  if (algorithm == "structure_only_3") return 3;
  if (algorithm == "structure_only_2") return 2;
  return 0;
}

// StructureOnlySolver<PointDoF> asserts v->dimension() == PointDoF (:81): a name that does not match the graph's
// marginalised vertices is refused
void Engine::so_check_dim() const {
  const int want = so_name_dim(algorithm);
  if (!want) return;
  for (int vi : active) {
    const HVertex& v = hg.verts[vi];
    if (v.marg && v.dim != want)
      throw StatusError(G2OHIP_ERR_UNSUPPORTED, algorithm + ": marginalised vertex " + std::to_string(v.id) +
                                                    " has dimension " + std::to_string(v.dim));
  }
}

// The groups calc reads. StructureOnlySolver::calc walks v->edges() (:82): every edge of the landmark whatever its
// level. Without a level filter these are `groups`; with one, groups of every edge (same per-landmark edge order,
// same conversion), kept beside the active ones and rebuilt with them
const std::vector<EGroup>& Engine::so_groups() {
  if (!level_filtered_) {
    so_all_groups_.clear();
    so_all_key_ = 0;
    return groups;
  }
  if (so_all_key_ != edges_ver) {
    form_groups(false, so_all_groups_);
    for (EGroup& g : so_all_groups_) fill_group_device(g);
    so_all_key_ = edges_ver;
  }
  return so_all_groups_;
}

// init() (:214-225): the active vertices with marginalized() set, fixed ones included, in id order; per landmark the
// edges of v->edges() as (group, edge) entries, by group and then by the group's edge order
void Engine::so_build_list() {
  if (so_.key == edges_ver) return;
  const std::vector<EGroup>& groups = so_groups();
  SoList& L = so_;
  L.refuse.clear();
  L.lm_of_vertex.assign(hg.verts.size(), -1);
  L.group_of.clear();
  std::vector<int> local;
  std::vector<unsigned char> fixed;
  L.ld = L.vt = 0;
  for (int vi : active) {
    const HVertex& v = hg.verts[vi];
    if (!v.marg) continue;
    if (v.type != G2OHIP_V_XYZ && v.type != G2OHIP_V_XY)
      throw StatusError(G2OHIP_ERR_UNSUPPORTED, "structure-only: marginalised vertex " + std::to_string(v.id) +
                                                    " of vertex type " + std::to_string(v.type) + " is no point");
    if (L.vt && L.vt != v.type)
      throw StatusError(G2OHIP_ERR_UNSUPPORTED, "structure-only: marginalised vertices of two point types");
    L.vt = v.type;
    L.ld = v.dim;
    L.lm_of_vertex[vi] = (int)local.size();
    local.push_back(v.local);
    fixed.push_back(v.fixed ? 1 : 0);
  }
  L.nlm = (int)local.size();
  // the landmark end of each group (EdgeTypeInfo::lm): v0 for the BA and sba types, Edge_XYZ_VSC and the point priors, v1
  // for slam3d, SE2-XY and the bearing edge; LM_NONE: the other types, the host-J ones, and the landmark edges whose
  // family k_structure_only has no term for (has_structure_only_form: EdgeObservationBAL)
  auto lm_side = [&](const EGroup& g) {
    const EdgeTypeInfo* t = edge_type_info(hg.esets[g.set].type);
    return t && has_structure_only_form(t->family) ? t->lm : LM_NONE;
  };
  std::vector<int> cnt(L.nlm + 1, 0);
  std::vector<int> gslot(groups.size(), -1);
  auto lm_end = [&](const EGroup& g, int k) {  // vertex index of the edge's marginalised endpoint(s): (a, b), -1 none
    const HEdgeSet& es = hg.esets[g.set];
    const int e = g.edges[k];
    const int a = es.ev0[e], b = es.v1(e);
    return std::pair<int, int>{L.lm_of_vertex[a] >= 0 ? a : -1, b >= 0 && L.lm_of_vertex[b] >= 0 ? b : -1};
  };
  for (size_t gi = 0; gi < groups.size() && L.nlm; ++gi) {
    const EGroup& g = groups[gi];
    const bool lm_first = lm_side(g) == LM_V0, lm_second = lm_side(g) == LM_V1;
    for (int k = 0; k < g.ne; ++k) {
      const auto [a, b] = lm_end(g, k);
      if (a < 0 && b < 0) continue;
      if (is_hostj_family(g.family)) {
        L.refuse = "structure-only: landmark " + std::to_string(hg.verts[a >= 0 ? a : b].id) +
                   " carries a host-Jacobian edge (type " + std::to_string(hg.esets[g.set].type) + ")";
        continue;
      }
      if (!(lm_first && a >= 0) && !(lm_second && b >= 0))
        throw StatusError(G2OHIP_ERR_UNSUPPORTED, "structure-only: edge type " + std::to_string(hg.esets[g.set].type) +
                                                      " on a marginalised vertex");
      if (gslot[gi] < 0) {
        gslot[gi] = (int)L.group_of.size();
        L.group_of.push_back((int)gi);
      }
      ++cnt[L.lm_of_vertex[lm_first ? a : b] + 1];
    }
  }
  std::partial_sum(cnt.begin(), cnt.end(), cnt.begin());
  L.nent = cnt.back();
  std::vector<int2> ent(std::max<size_t>((size_t)L.nent, 1), int2{0, 0});
  std::vector<int> fill(cnt.begin(), cnt.end() - 1);
  for (int gi : L.group_of) {
    const EGroup& g = groups[gi];
    const bool lm_first = lm_side(g) == LM_V0;
    for (int k = 0; k < g.ne; ++k) {
      const auto [a, b] = lm_end(g, k);
      const int v = lm_first ? a : b;
      if (v < 0) continue;
      ent[fill[L.lm_of_vertex[v]]++] = int2{gslot[gi], k};
    }
  }
  // one family over every entry: the templated kernel where it exists
  L.single_family = -1;
  if (L.group_of.size() == 1) {
    const int f = groups[L.group_of[0]].family;
    if (f == FAM_BA || f == FAM_SE2XY) L.single_family = f;
  }
  if (local.empty()) { local.push_back(0); fixed.push_back(1); }
  L.ptr.upload(cnt, stream);
  L.ent.upload(ent, stream);
  L.local.upload(local, stream);
  L.fixed.upload(fixed, stream);
  L.key = edges_ver;
}

int Engine::structure_only_calc(int n, const int* ids, int num_iters, int num_max_trials, long long* counts) {
  if (!initialized) return G2OHIP_ERR_STATE;
  if (num_iters < 0 || num_max_trials < 1 || (ids && n < 0))
    throw StatusError(G2OHIP_ERR_ARG, "structure-only: num_iters >= 0 and num_max_trials >= 1 (and n >= 0 ids)");
  if (nranks > 1)
    throw StatusError(G2OHIP_ERR_UNSUPPORTED, "structure-only on a sharded graph (nranks > 1) is not supported");
  so_check_dim();
  ensure_device_state();
  if (!edges_ready) setup_edges_device();
  so_build_list();
  SoList& L = so_;
  if (!L.refuse.empty()) throw StatusError(G2OHIP_ERR_UNSUPPORTED, L.refuse);
  if (counts) std::fill(counts, counts + launch::SO_COUNTS, 0LL);
  int nsel = L.nlm;
  if (ids) {  // every id a marginalised active vertex, none twice (each landmark belongs to one lane group)
    std::vector<int> sel(n);
    std::vector<char> seen(L.nlm, 0);
    for (int k = 0; k < n; ++k) {
      const auto it = hg.idmap.find(ids[k]);
      const int l = it == hg.idmap.end() ? -1 : L.lm_of_vertex[it->second];
      if (l < 0) throw StatusError(G2OHIP_ERR_ARG, "structure-only: vertex " + std::to_string(ids[k]) + " is no landmark");
      if (seen[l]) throw StatusError(G2OHIP_ERR_ARG, "structure-only: landmark " + std::to_string(ids[k]) + " given twice");
      seen[l] = 1;
      sel[k] = l;
    }
    nsel = n;
    if (nsel) L.sel.upload(sel, stream);
  }
  if (nsel == 0) return G2OHIP_OK;  // no marginalised vertex: OK and nothing done (:78 loops over an empty set)
  const std::vector<EGroup>& groups = so_groups();
  std::vector<launch::SoGroup> sg(std::max<size_t>(L.group_of.size(), 1));
  std::memset(sg.data(), 0, sizeof(launch::SoGroup) * sg.size());
  for (size_t k = 0; k < L.group_of.size(); ++k) {
    const EGroup& g = groups[L.group_of[k]];
    const bool lm_first = edge_type_info(hg.esets[g.set].type)->lm == LM_V0;  // (a listed group has a landmark end)
    launch::SoGroup& o = sg[k];
    o.vo = is_unary_family(g.family) ? nullptr : (lm_first ? g.v1.get() : g.v0.get());
    const int vto = lm_first ? g.vtB : g.vtA;
    o.so = is_unary_family(g.family) ? nullptr : dstate[vto].get();
    o.meas = g.meas.get();
    o.info = g.info.get();
    o.params = g.params.get();
    o.rk = hg.esets[g.set].rk;
    o.rk_delta = hg.esets[g.set].rk_delta;
    o.ue = g.ue;
    o.family = g.family;
  }
  L.groups.upload(sg, stream);
  const int nb = launch::so_blocks(nsel);
  L.part.resize((size_t)nb * launch::SO_COUNTS);
  launch::SoCall c{L.groups.get(), L.ptr.get(), L.ent.get(), L.local.get(), L.fixed.get(), ids ? L.sel.get() : nullptr,
                   nsel, dstate[L.vt].get(), num_iters, num_max_trials, L.part.get()};
  timer.begin("structure_only", stream);
  launch::structure_only(L.ld, L.single_family, c, stream);
  timer.end(stream);
  // the landmarks moved: the chi2 cache, the assembled system (built_ver), the dogleg's cached chi2 (chi_ver) and the
  // Schur split's records (fz_lambda: +inf never equals a trial's lambda, so the next solve re-assembles, and
  // ensure_hpp still sees a split assembly) belong to the old state. The push / pop stacks are not touched.
  host_state_stale = true;
  ++state_ver;
  built_ver = 0;
  if (!std::isnan(fz_lambda)) fz_lambda = std::numeric_limits<double>::infinity();
  std::vector<long long> part((size_t)nb * launch::SO_COUNTS);
  L.part.download(part.data(), part.size(), stream);
  HIP_CHECK(hipStreamSynchronize(stream));
  timer.collect();
  if (counts)
    for (int b = 0; b < nb; ++b)  // block order
      for (int k = 0; k < launch::SO_COUNTS; ++k) counts[k] += part[(size_t)b * launch::SO_COUNTS + k];
  return G2OHIP_OK;
}

// StructureOnlySolver::solve (:65-70): calc(_points, 1), always OK
int Engine::so_solve() {
  if (int r = structure_only_calc(0, nullptr, 1, 10, nullptr)) return r;
  levenberg_iterations = 0;
  return 0;
}

}  // namespace g2ohip
