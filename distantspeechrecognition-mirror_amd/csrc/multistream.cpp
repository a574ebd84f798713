// csrc/multistream.cpp -- the host side of multi-stream decoding (include/dsr.h section 8b): DistribMap (asr/gaussian/distribBasic.h:390-408,
// distribBasic.cc:326-376), the combiner of two models' scores (DistribMultiStream, distribBasic.h:135-158) with the name resolution of the
// DistribSetMultiStream constructors (distribBasic.cc:381-410), and the multi-stream distribution set.  The arithmetic is ms_kernels.hip's alone.
#include "multistream.h"
#include "befile.h"

using namespace dsr;

struct dsr_distribmap { std::map<std::string, std::string> m; };

namespace {
constexpr size_t kMaxName = 19;                                     // the reference reads into char[20] (distribBasic.cc:338-339)
void name_fits(const std::string& s)
{ if (s.size() > kMaxName) throw Error(DSR_E_PARAMETER, "distribution name %s has more than %zu characters", s.c_str(), kMaxName); }
const std::string& mapped(const dsr_distribmap* m, const std::string& name)
{
  std::map<std::string, std::string>::const_iterator it = m->m.find(name);
  if (it == m->m.end()) throw Error(DSR_E_INDEX, "No mapping for %s", name.c_str());                    // distribBasic.cc:353-354
  return it->second;
}
}  // namespace

extern "C" {

dsr_status dsr_distribmap_create(dsr_distribmap** out)
{ return guard([&] { if (!out) throw Error(DSR_E_PARAMETER, "null argument"); *out = new dsr_distribmap(); }); }
void dsr_distribmap_destroy(dsr_distribmap* m) { delete m; }
dsr_status dsr_distribmap_add(dsr_distribmap* m, const char* from, const char* to)
{
  return guard([&] {
    if (!m || !from || !to) throw Error(DSR_E_PARAMETER, "null argument");
    name_fits(from); name_fits(to);
    m->m[from] = to;
  });
}
dsr_status dsr_distribmap_mapped(const dsr_distribmap* m, const char* name, const char** to)
{ return guard([&] { if (!m || !name || !to) throw Error(DSR_E_PARAMETER, "null argument"); *to = mapped(m, name).c_str(); }); }
int dsr_distribmap_size(const dsr_distribmap* m) { return m ? (int) m->m.size() : 0; }
dsr_status dsr_distribmap_read(dsr_distribmap* m, const char* fileName)
{
  return guard([&] {
    if (!m || !fileName) throw Error(DSR_E_PARAMETER, "null argument");
    if (!*fileName) throw Error(DSR_E_ERROR, "Distribution map file name is null.");
    BEFile f(fileName, "rb");
    const int n = f.i32(); if (n < 0) throw Error(DSR_E_IO, "bad pair count %d", n);
    std::map<std::string, std::string> pairs;
    for (int i = 0; i < n; i++) {
      const std::string from = f.str(), to = f.str();
      name_fits(from); name_fits(to);
      pairs[from] = to;
    }
    m->m.swap(pairs);                                                                                    // distribBasic.cc:337: read clears first
  });
}
dsr_status dsr_distribmap_write(const dsr_distribmap* m, const char* fileName)
{
  return guard([&] {
    if (!m || !fileName) throw Error(DSR_E_PARAMETER, "null argument");
    if (!*fileName) throw Error(DSR_E_ERROR, "Distribution map file name is null.");
    for (std::map<std::string, std::string>::const_iterator it = m->m.begin(); it != m->m.end(); ++it) { name_fits(it->first); name_fits(it->second); }
    BEFile f(fileName, "wb");
    f.w32((int) m->m.size());
    for (std::map<std::string, std::string>::const_iterator it = m->m.begin(); it != m->m.end(); ++it) { f.wstr(it->first); f.wstr(it->second); }
  });
}

dsr_status dsr_ms_create(const dsr_gmm* audio, const dsr_gmm* video, const dsr_distribmap* map, double audioWeight, double videoWeight, dsr_ms** out)
{
  return guard([&] {
    if (!audio || !video || !out) throw Error(DSR_E_PARAMETER, "null argument");
    std::unique_ptr<dsr_ms> ms(new dsr_ms()); ms->KA = dsr_gmm_num_dists(audio); ms->KV = dsr_gmm_num_dists(video); ms->wA = audioWeight; ms->wV = videoWeight;
    std::map<std::string, int> videoX;
    for (int k = ms->KV - 1; k >= 0; k--) videoX[dsr_gmm_dist_name(video, k)] = k;                       // find() gives the first of a repeated name
    ms->table.resize((size_t) ms->KA);
    for (int k = 0; k < ms->KA; k++) {                                                                   // distribBasic.cc:385-391, 400-409
      const std::string name = dsr_gmm_dist_name(audio, k);
      const std::string& partner = map ? mapped(map, name) : name;
      std::map<std::string, int>::const_iterator it = videoX.find(partner);
      if (it == videoX.end()) throw Error(DSR_E_KEY, "Could not find key %s in the video distribution set", partner.c_str());
      ms->table[(size_t) k] = it->second;
    }
    require_device();
    ms->d_table.upload(ms->table.data(), ms->table.size());
    *out = ms.release();
  });
}
void dsr_ms_destroy(dsr_ms* ms) { delete ms; }
dsr_status dsr_ms_set_weights(dsr_ms* ms, double audioWeight, double videoWeight)
{ return guard([&] { if (!ms) throw Error(DSR_E_PARAMETER, "null argument"); ms->wA = audioWeight; ms->wV = videoWeight; }); }
dsr_status dsr_ms_get_weights(const dsr_ms* ms, double* audioWeight, double* videoWeight)
{ return guard([&] { if (!ms || !audioWeight || !videoWeight) throw Error(DSR_E_PARAMETER, "null argument"); *audioWeight = ms->wA; *videoWeight = ms->wV; }); }
dsr_status dsr_ms_table(const dsr_ms* ms, int32_t* table)
{ return guard([&] { if (!ms || !table) throw Error(DSR_E_PARAMETER, "null argument"); if (ms->KA) memcpy(table, ms->table.data(), sizeof(int32_t) * (size_t) ms->KA); }); }
dsr_status dsr_ms_combine(dsr_ms* ms, const float* sA_dev, const float* sV_dev, int64_t N, float* out_dev, void* stream)
{
  return guard([&] {
    if (!ms || !sA_dev || !sV_dev || !out_dev) throw Error(DSR_E_PARAMETER, "null argument");
    if (N < 0) throw Error(DSR_E_PARAMETER, "%lld frames", (long long) N);
    if (out_dev == sV_dev) throw Error(DSR_E_PARAMETER, "the output may be the audio matrix, never the video matrix");
    ms_combine(sA_dev, sV_dev, ms->d_table.p, N, ms->KA, ms->KV, ms->wA, ms->wV, out_dev, (hipStream_t) stream);
  });
}
dsr_status dsr_ms_combine_path(int KA, int KV, int aligned16, int* path, int* rowsPerTile, int64_t* ldsBytes)
{
  return guard([&] {
    if (!path || !rowsPerTile || !ldsBytes) throw Error(DSR_E_PARAMETER, "null argument");
    if (KA < 1 || KV < 1) throw Error(DSR_E_PARAMETER, "%d audio and %d video states", KA, KV);
    const MsPath p = ms_path(KA, KV, aligned16 != 0);
    *path = p.path; *rowsPerTile = p.rows; *ldsBytes = p.ldsBytes;
  });
}

dsr_status dsr_distribset_create_multistream(dsr_distribset* audioSet, dsr_distribset* videoSet, const dsr_distribmap* map, double audioWeight,
                                             double videoWeight, dsr_distribset** out)
{
  return guard([&] {
    if (!audioSet || !videoSet || !out) throw Error(DSR_E_PARAMETER, "null argument");
    if (audioSet->ms || videoSet->ms) throw Error(DSR_E_TYPE, "the children of a multi-stream set are plain distribution sets");
    std::unique_ptr<dsr_distribset> d(new dsr_distribset());
    const dsr_status st = dsr_ms_create(audioSet->gmm, videoSet->gmm, map, audioWeight, videoWeight, &d->ms);
    if (st) throw Error(st, "%s", dsr_last_error());
    d->audio = audioSet; d->video = videoSet; audioSet->refs++; videoSet->refs++;
    *out = d.release();
  });
}
dsr_status dsr_distribset_set_weights(dsr_distribset* d, double audioWeight, double videoWeight)
{
  return guard([&] {
    if (!d) throw Error(DSR_E_PARAMETER, "null argument");
    if (!d->ms) throw Error(DSR_E_TYPE, "not a multi-stream distribution set");
    d->ms->wA = audioWeight; d->ms->wV = videoWeight; d->cachedFrame = -1;
  });
}
dsr_status dsr_distribset_get_weights(const dsr_distribset* d, double* audioWeight, double* videoWeight)
{
  return guard([&] {
    if (!d || !audioWeight || !videoWeight) throw Error(DSR_E_PARAMETER, "null argument");
    if (!d->ms) throw Error(DSR_E_TYPE, "not a multi-stream distribution set");
    *audioWeight = d->ms->wA; *videoWeight = d->ms->wV;
  });
}

}  // extern "C"
