// csrc/befile.h -- the big-endian binary files of the reference (btk/common/mach_ind_io.cc:176-510: read_int / read_float / read_string and
// their writers), as train.cpp and fsat.cpp (accumulator files) and fsa.cpp (SAS / SAW files) share them.
#pragma once
#include "common.h"
#include <map>
#include <string>

namespace dsr {

struct BEFile {
  FILE* fp = nullptr;
  BEFile(const char* name, const char* mode) { fp = fopen(name, mode); if (!fp) throw Error(DSR_E_IO, "Could not open file %s.", name); }
  ~BEFile() { if (fp) fclose(fp); }
  int i32() { unsigned char b[4] = {0, 0, 0, 0}; if (fread(b, 1, 4, fp) != 4) throw Error(DSR_E_IO, "premature end of file"); return (int) ((unsigned) b[0] << 24 | (unsigned) b[1] << 16 | (unsigned) b[2] << 8 | (unsigned) b[3]); }
  float f32() { int i = i32(); float f; memcpy(&f, &i, 4); return f; }
  std::string str()
  {
    unsigned char b[2] = {0, 0}; if (fread(b, 1, 2, fp) != 2) throw Error(DSR_E_IO, "premature end of file");
    const int len = (short) ((unsigned) b[0] << 8 | (unsigned) b[1]); if (len < 0) throw Error(DSR_E_IO, "bad string length %d", len);
    std::string s((size_t) len + 1, '\0'); if (fread(&s[0], (size_t) len + 1, 1, fp) != 1) throw Error(DSR_E_IO, "premature end of file");
    s.resize(len); return s;
  }
  void w32(int v) { unsigned u = (unsigned) v; unsigned char b[4] = { (unsigned char) (u >> 24), (unsigned char) (u >> 16), (unsigned char) (u >> 8), (unsigned char) u }; fwrite(b, 1, 4, fp); }
  void wf(float f) { int i; memcpy(&i, &f, 4); w32(i); }
  bool magic(const char* m) { char b[3]; return fread(b, 1, 3, fp) == 3 && strncmp(m, b, 3) == 0; }      // a three-byte tag without a length
  void wstr(const std::string& s) { unsigned short u = (unsigned short) s.size(); unsigned char b[2] = { (unsigned char) (u >> 8), (unsigned char) u }; fwrite(b, 1, 2, fp); fwrite(s.c_str(), s.size() + 1, 1, fp); }
};

// the directory in front of an accumulator file (AccMap, asr/train/distribTrain.cc "dT"), as train.cpp and fsat.cpp share it
const char* const kEndOfAccs = "EndOfAccumulators";       // distribTrain.h:230-233
const int kCbMarker = 123456789, kDsMarker = 987654321;   // codebookTrain.cc:309, dT:264
const int kCovDiagonal = 2;

inline std::map<std::string, long> read_map(BEFile& f)    // AccMap::AccMap(FILE*), dT:343-355
{
  std::map<std::string, long> m;
  for (;;) {
    const std::string name = f.str(); if (name == kEndOfAccs) break;
    if (m.count(name)) throw Error(DSR_E_KEY, "State map name %s is not unique.", name.c_str());
    m[name] = f.i32();
  }
  return m;
}
inline void write_map(BEFile& f, const std::map<std::string, long>& m)   // AccMap::write, dT:400-411: std::map order
{
  for (std::map<std::string, long>::const_iterator it = m.begin(); it != m.end(); ++it) { f.wstr(it->first); f.w32((int) it->second); }
  f.wstr(kEndOfAccs);
}

}  // namespace dsr
