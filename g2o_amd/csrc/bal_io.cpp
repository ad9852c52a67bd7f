// The "Bundle Adjustment in the Large" text format, as examples/bal/bal_example.cpp:336-406 reads it:
//   ncams npts nobs | nobs records "cam pt x y" | 9 * ncams camera values | 3 * npts point values
// with whitespace of any kind between the tokens. Engine::load_bal / Engine::save_bal (g2ohip_load_bal / g2ohip_save_bal).
#include <cctype>
#include <cerrno>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "engine.hpp"

namespace g2ohip {
namespace {

// whitespace-separated tokens of one buffer; a failed read names the record it was in
struct BalCursor {
  const char* p;
  const char* e;
  std::string path;
  [[noreturn]] void fail(const std::string& what, const std::string& record) const {
    throw StatusError(G2OHIP_ERR_ARG, "g2ohip_load_bal: " + path + ": " + what + " in " + record);
  }
  // the next token's bounds; false at the end of the file
  bool token(const char*& b, const char*& t) {
    while (p < e && std::isspace((unsigned char)*p)) ++p;
    if (p >= e) return false;
    b = p;
    while (p < e && !std::isspace((unsigned char)*p)) ++p;
    t = p;
    return true;
  }
  long long integer(const std::string& record) {
    const char *b, *t;
    if (!token(b, t)) fail("the file ends", record);
    const std::string s(b, t);
    char* end = nullptr;
    errno = 0;
    const long long v = std::strtoll(s.c_str(), &end, 10);
    if (end == s.c_str() || *end != '\0' || errno == ERANGE) fail("non-numeric token '" + s + "'", record);
    return v;
  }
  double real(const std::string& record) {
    const char *b, *t;
    if (!token(b, t)) fail("the file ends", record);
    const std::string s(b, t);
    // decimal numbers only: strtod would also take "nan", "inf" and hexadecimal floats
    const size_t d = s[0] == '+' || s[0] == '-' ? 1 : 0;
    const bool decimal = d < s.size() && (std::isdigit((unsigned char)s[d]) || s[d] == '.') &&
                         s.find_first_of("xXpP") == std::string::npos;
    char* end = nullptr;
    const double v = decimal ? std::strtod(s.c_str(), &end) : 0.0;
    if (!decimal || end == s.c_str() || *end != '\0') fail("non-numeric token '" + s + "'", record);
    if (!std::isfinite(v)) fail("token '" + s + "' is no finite number", record);
    return v;
  }
};

}  // namespace

int Engine::load_bal(const char* path, int marginalize_points) {
  FILE* f = fopen(path, "rb");
  if (!f) throw StatusError(G2OHIP_ERR_ARG, std::string("g2ohip_load_bal: cannot open ") + path);
  std::vector<char> buf;
  {
    char chunk[1 << 16];
    size_t n;
    while ((n = fread(chunk, 1, sizeof chunk, f)) > 0) buf.insert(buf.end(), chunk, chunk + n);
    fclose(f);
  }
  BalCursor c{buf.data(), buf.data() + buf.size(), path};
  // everything is parsed and checked before the graph is touched: a bad file leaves it as it was
  const long long ncams = c.integer("the header (ncams npts nobs)"), npts = c.integer("the header (ncams npts nobs)"),
                  nobs = c.integer("the header (ncams npts nobs)");
  if (ncams < 0 || npts < 0 || nobs < 0 || ncams + npts > 0x7fffffffLL || nobs > 0x7fffffffLL)
    c.fail("a negative or oversized count", "the header (ncams npts nobs)");
  // nothing is allocated from counts the file cannot hold: an observation takes at least 8 bytes ("0 0 0 0 "), a value 2
  if (8 * nobs + 2 * (9 * ncams + 3 * npts) > (long long)(c.e - c.p) + 1)
    c.fail("counts " + std::to_string(ncams) + " " + std::to_string(npts) + " " + std::to_string(nobs) +
               " that the file is too short for",
           "the header (ncams npts nobs)");
  std::vector<int> ec((size_t)nobs), ep((size_t)nobs);
  std::vector<double> meas((size_t)nobs * 2);
  for (long long k = 0; k < nobs; ++k) {
    const std::string rec = "observation " + std::to_string(k);
    const long long ci = c.integer(rec), pi = c.integer(rec);
    if (ci < 0 || ci >= ncams) c.fail("camera index " + std::to_string(ci) + " out of range [0, " + std::to_string(ncams) + ")", rec);
    if (pi < 0 || pi >= npts) c.fail("point index " + std::to_string(pi) + " out of range [0, " + std::to_string(npts) + ")", rec);
    ec[k] = (int)ci;
    ep[k] = (int)(ncams + pi);  // bal_example.cpp:345-364: the points' ids follow the cameras'
    meas[2 * k] = c.real(rec);
    meas[2 * k + 1] = c.real(rec);
  }
  std::vector<double> cams((size_t)ncams * 9), pts((size_t)npts * 3);
  for (long long k = 0; k < ncams; ++k)
    for (int j = 0; j < 9; ++j) cams[k * 9 + j] = c.real("camera " + std::to_string(k));
  for (long long k = 0; k < npts; ++k)
    for (int j = 0; j < 3; ++j) pts[k * 3 + j] = c.real("point " + std::to_string(k));
  for (long long id = 0; id < ncams + npts; ++id)
    if (hg.idmap.count((int)id))
      throw StatusError(G2OHIP_ERR_ARG, "g2ohip_load_bal: the graph already holds a vertex with id " + std::to_string(id) +
                                            " (the file's cameras take 0 .. ncams-1, its points the ids behind them)");
  std::vector<int> cid((size_t)ncams), pid((size_t)npts), marg((size_t)npts, marginalize_points ? 1 : 0);
  for (long long k = 0; k < ncams; ++k) cid[k] = (int)k;
  for (long long k = 0; k < npts; ++k) pid[k] = (int)(ncams + k);
  std::vector<double> info((size_t)nobs * 4, 0.0);  // the identity (:391); equal records share one on the device
  for (long long k = 0; k < nobs; ++k) info[4 * k] = info[4 * k + 3] = 1.0;
  // after the checks above none of the three calls has a reason to fail; should one, the vertices appended so far are
  // taken off again (they are the last of the graph), so that the graph is left as it was in that case too
  const size_t nv0 = hg.verts.size();
  auto roll_back = [&] {
    while (hg.verts.size() > nv0) {
      const HVertex& v = hg.verts.back();
      hg.idmap.erase(v.id);
      hg.by_type[v.type].pop_back();
      hg.st[v.type].resize(hg.st[v.type].size() - (size_t)vertex_state_stride(v.type));
      hg.verts.pop_back();
    }
  };
  int r = G2OHIP_OK;
  try {
    r = add_vertices(G2OHIP_V_CAM_BAL, (int)ncams, cid.data(), cams.data(), nullptr, nullptr);
    if (!r) r = add_vertices(G2OHIP_V_XYZ, (int)npts, pid.data(), pts.data(), nullptr, marg.data());
    if (!r) r = add_edges(G2OHIP_E_OBSERVATION_BAL, (int)nobs, ec.data(), ep.data(), meas.data(), info.data(), nullptr);
  } catch (...) {
    roll_back();
    throw;
  }
  if (r) roll_back();
  return r;
}

int Engine::save_bal(const char* path) {
  const char* fn = "g2ohip_save_bal: ";
  const int ncams = (int)hg.by_type[G2OHIP_V_CAM_BAL].size(), npts = (int)hg.by_type[G2OHIP_V_XYZ].size();
  if ((size_t)(ncams + npts) != hg.verts.size())
    throw StatusError(G2OHIP_ERR_UNSUPPORTED, std::string(fn) + "the graph holds vertices other than VertexCameraBAL "
                                                  "and VertexPointBAL (G2OHIP_V_CAM_BAL, G2OHIP_V_XYZ)");
  for (const HEdgeSet& es : hg.esets)
    if (es.type != G2OHIP_E_OBSERVATION_BAL && !es.ev0.empty())
      throw StatusError(G2OHIP_ERR_UNSUPPORTED, std::string(fn) + "the graph holds edges of type " +
                                                    std::to_string(es.type) + ", the format carries EdgeObservationBAL only");
  // ids of the shape the reader gives: camera k has id k, point k id ncams + k, in insertion order
  for (int k = 0; k < ncams; ++k)
    if (hg.verts[hg.by_type[G2OHIP_V_CAM_BAL][k]].id != k)
      throw StatusError(G2OHIP_ERR_UNSUPPORTED, std::string(fn) + "camera " + std::to_string(k) + " has id " +
                                                    std::to_string(hg.verts[hg.by_type[G2OHIP_V_CAM_BAL][k]].id) +
                                                    ": the format numbers the cameras 0 .. ncams-1");
  for (int k = 0; k < npts; ++k)
    if (hg.verts[hg.by_type[G2OHIP_V_XYZ][k]].id != ncams + k)
      throw StatusError(G2OHIP_ERR_UNSUPPORTED, std::string(fn) + "point " + std::to_string(k) + " has id " +
                                                    std::to_string(hg.verts[hg.by_type[G2OHIP_V_XYZ][k]].id) +
                                                    ": the format numbers the points ncams .. ncams+npts-1");
  const HEdgeSet* es = hg.set_of(G2OHIP_E_OBSERVATION_BAL);
  const size_t nobs = es ? es->ev0.size() : 0;
  for (size_t k = 0; k < nobs; ++k)
    for (int j = 0; j < 4; ++j)
      if (es->info[k * 4 + j] != (j == 0 || j == 3 ? 1.0 : 0.0))
        throw StatusError(G2OHIP_ERR_UNSUPPORTED, std::string(fn) + "observation " + std::to_string(k) +
                                                      " has an information matrix other than the identity, which the "
                                                      "format cannot carry");
  sync_host_state();
  // the whole text first: nothing is written unless all of it can be
  std::string out;
  char line[128];
  snprintf(line, sizeof line, "%d %d %zu\n", ncams, npts, nobs);
  out += line;
  for (size_t k = 0; k < nobs; ++k) {
    snprintf(line, sizeof line, "%d %d %.17g %.17g\n", hg.verts[es->ev0[k]].id, hg.verts[es->ev1[k]].id - ncams,
             es->meas[2 * k], es->meas[2 * k + 1]);
    out += line;
  }
  for (int k = 0; k < ncams; ++k)
    for (int j = 0; j < 9; ++j) {
      snprintf(line, sizeof line, "%.17g\n", hg.st[G2OHIP_V_CAM_BAL][(size_t)k * 9 + j]);
      out += line;
    }
  for (int k = 0; k < npts; ++k)
    for (int j = 0; j < 3; ++j) {
      snprintf(line, sizeof line, "%.17g\n", hg.st[G2OHIP_V_XYZ][(size_t)k * 3 + j]);
      out += line;
    }
  FILE* f = fopen(path, "wb");
  if (!f) throw StatusError(G2OHIP_ERR_ARG, std::string(fn) + "cannot open " + path);
  const bool ok = fwrite(out.data(), 1, out.size(), f) == out.size();
  if (fclose(f) != 0 || !ok) throw StatusError(G2OHIP_ERR_ARG, std::string(fn) + "writing " + path + " failed");
  return G2OHIP_OK;
}

}  // namespace g2ohip
