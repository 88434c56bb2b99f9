// The vocabulary of the loop detector (vpl_ld_*): the reference's binary file (pose_graph/src/ThirdParty/VocabularyBinary.hpp,
// read by TemplatedVocabulary::loadBin, TemplatedVocabulary.h:1509-1561), its validation, and the flat layout the descent walks
// -- one description for the host and the device.  Plain C++ (no HIP): tests/native/ld_vocab_check.cpp compiles it alone.
//
// File: six int32 (k, L, scoringType, weightingType, nNodes, nWords); nNodes records of 48 bytes (int32 nodeId, int32 parentId,
// double weight, uint64 descriptor[4]); nWords records of 8 bytes (int32 nodeId, int32 wordId).  The root is node 0 and not in
// the file.  A node's children are in file order.
//
// Flat layout: the nodes in breadth-first order, the root at 0, the children of a node in ONE RUN in file order, so that a step
// of the descent reads `childCount` consecutive 32-byte descriptors from `childBegin`.  The descent (transform,
// TemplatedVocabulary.h:1217-1258) starts at 0, goes to the child of least Hamming distance (the first one on a tie) and stops
// at the first node without children; `word` of that node is its word id, `wordWeight` of the word its weight.
#pragma once
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

namespace vpl {

constexpr int LD_MAX_DEPTH = 16;        // levels below the root a vocabulary may have
constexpr int LD_SCORING_L1 = 0;        // DBoW2::ScoringType L1_NORM, the only one taken
constexpr int LD_TF_IDF = 0, LD_TF = 1, LD_IDF = 2, LD_BINARY = 3;   // DBoW2::WeightingType

struct LdVocabRaw {   // the arrays of vpl_ld_set_vocabulary, the content of the file
  int k = 0, L = 0, scoring = 0, weighting = 0;
  std::vector<int> nodeId, parentId;
  std::vector<double> weight;
  std::vector<uint64_t> desc;            // [nNodes][4]
  std::vector<int> wordNode, wordId;
};

struct LdVocabFlat {
  int k = 0, L = 0, scoring = 0, weighting = 0;
  int nFlat = 1, nWords = 0, depth = 0;  // nodes with the root | words | deepest level
  std::vector<int> childBegin, childCount, word, nodeOf;   // [nFlat]; word -1 on inner nodes; nodeOf: the file's node id
  std::vector<uint64_t> desc;            // [nFlat][4]
  std::vector<double> wordWeight;        // [nWords]
};

inline bool ld_write_file(const char* path, const LdVocabRaw& v, std::string& err) {
  FILE* f = std::fopen(path, "wb");
  if (!f) { err = std::string("cannot write ") + path; return false; }
  const int32_t hdr[6] = {v.k, v.L, v.scoring, v.weighting, (int32_t)v.nodeId.size(), (int32_t)v.wordId.size()};
  bool ok = std::fwrite(hdr, 4, 6, f) == 6;
  for (size_t i = 0; ok && i < v.nodeId.size(); ++i) {
    unsigned char rec[48];
    const int32_t ids[2] = {v.nodeId[i], v.parentId[i]};
    std::memcpy(rec, ids, 8); std::memcpy(rec + 8, &v.weight[i], 8); std::memcpy(rec + 16, &v.desc[4 * i], 32);
    ok = std::fwrite(rec, 48, 1, f) == 1;
  }
  for (size_t i = 0; ok && i < v.wordId.size(); ++i) {
    const int32_t rec[2] = {v.wordNode[i], v.wordId[i]};
    ok = std::fwrite(rec, 8, 1, f) == 1;
  }
  ok = (std::fclose(f) == 0) && ok;
  if (!ok) err = std::string("write to ") + path + " failed";
  return ok;
}

inline bool ld_read_file(const char* path, LdVocabRaw& v, std::string& err) {
  FILE* f = std::fopen(path, "rb");
  if (!f) { err = std::string("cannot open ") + path; return false; }
  struct Closer { FILE* f; ~Closer() { std::fclose(f); } } closer{f};
  int32_t hdr[6];
  if (std::fread(hdr, 4, 6, f) != 6) { err = "vocabulary file truncated inside its header"; return false; }
  if (hdr[4] < 0 || hdr[5] < 0) { err = "vocabulary file: negative node or word count"; return false; }
  // the length first: a header that promises more than the file holds must not size an allocation
  if (std::fseek(f, 0, SEEK_END) != 0) { err = "vocabulary file: cannot seek"; return false; }
  const long long have = std::ftell(f), need = 24 + 48LL * hdr[4] + 8LL * hdr[5];
  if (have < need) {
    err = "vocabulary file truncated: " + std::to_string(have) + " bytes, " + std::to_string(need) + " needed for " +
          std::to_string(hdr[4]) + " nodes and " + std::to_string(hdr[5]) + " words";
    return false;
  }
  if (std::fseek(f, 24, SEEK_SET) != 0) { err = "vocabulary file: cannot seek"; return false; }
  const size_t n = hdr[4], w = hdr[5];
  v.k = hdr[0]; v.L = hdr[1]; v.scoring = hdr[2]; v.weighting = hdr[3];
  v.nodeId.resize(n); v.parentId.resize(n); v.weight.resize(n); v.desc.resize(4 * n); v.wordNode.resize(w); v.wordId.resize(w);
  std::vector<unsigned char> buf(48 * n);
  if (n && std::fread(buf.data(), 48, n, f) != n) { err = "vocabulary file truncated inside its nodes"; return false; }
  for (size_t i = 0; i < n; ++i) {
    const unsigned char* r = buf.data() + 48 * i;
    int32_t ids[2];
    std::memcpy(ids, r, 8); std::memcpy(&v.weight[i], r + 8, 8); std::memcpy(&v.desc[4 * i], r + 16, 32);
    v.nodeId[i] = ids[0]; v.parentId[i] = ids[1];
  }
  buf.resize(8 * w);
  if (w && std::fread(buf.data(), 8, w, f) != w) { err = "vocabulary file truncated inside its words"; return false; }
  for (size_t i = 0; i < w; ++i) {
    int32_t rec[2];
    std::memcpy(rec, buf.data() + 8 * i, 8);
    v.wordNode[i] = rec[0]; v.wordId[i] = rec[1];
  }
  return true;
}

// validates `v` and lays it out; on a refusal `out` is left as it was and `err` says why
inline bool ld_flatten(const LdVocabRaw& v, LdVocabFlat& out, std::string& err) {
  const size_t n = v.nodeId.size(), nw = v.wordId.size();
  if (v.parentId.size() != n || v.weight.size() != n || v.desc.size() != 4 * n || v.wordNode.size() != nw) {
    err = "vocabulary: arrays of different lengths"; return false;
  }
  if (n >= 0x7fffffffu || nw >= 0x7fffffffu) { err = "vocabulary: too many nodes"; return false; }
  if (v.scoring != LD_SCORING_L1) { err = "vocabulary: scoring " + std::to_string(v.scoring) + " is not L1_NORM (0), the only one taken"; return false; }
  if (v.weighting < LD_TF_IDF || v.weighting > LD_BINARY) { err = "vocabulary: weighting " + std::to_string(v.weighting) + " outside 0 .. 3"; return false; }
  // node ids 1 .. n, each once; parents 0 .. n
  std::vector<int> slot(n + 1, -1);      // file position by node id
  for (size_t i = 0; i < n; ++i) {
    const int id = v.nodeId[i], p = v.parentId[i];
    if (id < 1 || (size_t)id > n) { err = "vocabulary: node id " + std::to_string(id) + " outside 1 .. " + std::to_string(n); return false; }
    if (slot[id] >= 0) { err = "vocabulary: node id " + std::to_string(id) + " given twice"; return false; }
    if (p < 0 || (size_t)p > n) { err = "vocabulary: parent " + std::to_string(p) + " of node " + std::to_string(id) + " is not a node"; return false; }
    slot[id] = (int)i;
  }
  // children by parent, in file order
  std::vector<int> start(n + 2, 0), kids(n);
  for (size_t i = 0; i < n; ++i) start[v.parentId[i] + 1]++;
  for (size_t p = 0; p <= n; ++p) start[p + 1] += start[p];
  {
    std::vector<int> fill(start.begin(), start.end() - 1);
    for (size_t i = 0; i < n; ++i) kids[fill[v.parentId[i]]++] = v.nodeId[i];
  }
  // breadth first from the root: what it does not reach hangs on a cycle
  LdVocabFlat f;
  f.k = v.k; f.L = v.L; f.scoring = v.scoring; f.weighting = v.weighting;
  f.nFlat = (int)n + 1; f.nWords = (int)nw;
  f.childBegin.assign(n + 1, 0); f.childCount.assign(n + 1, 0); f.word.assign(n + 1, -1); f.nodeOf.assign(n + 1, 0);
  f.desc.assign(4 * (n + 1), 0); f.wordWeight.assign(nw, 0.0);
  std::vector<int> level(n + 1, 0), flatOf(n + 1, -1);
  flatOf[0] = 0;
  size_t next = 1;
  for (size_t at = 0; at < next; ++at) {
    const int node = f.nodeOf[at];
    f.childBegin[at] = (int)next; f.childCount[at] = start[node + 1] - start[node];
    for (int q = start[node]; q < start[node + 1]; ++q) {
      const int c = kids[q];
      if (level[at] + 1 > LD_MAX_DEPTH) { err = "vocabulary: node " + std::to_string(c) + " lies deeper than " + std::to_string(LD_MAX_DEPTH) + " levels"; return false; }
      f.nodeOf[next] = c; flatOf[c] = (int)next; level[next] = level[at] + 1;
      if (level[next] > f.depth) f.depth = level[next];
      std::memcpy(&f.desc[4 * next], &v.desc[4 * (size_t)slot[c]], 32);
      ++next;
    }
  }
  if (next != n + 1) {
    for (size_t id = 1; id <= n; ++id)
      if (flatOf[id] < 0) { err = "vocabulary: node " + std::to_string(id) + " is not reachable from the root (a cycle)"; return false; }
  }
  // words: on leaves, each id once, each leaf one
  std::vector<char> seen(nw, 0);
  for (size_t i = 0; i < nw; ++i) {
    const int node = v.wordNode[i], w = v.wordId[i];
    if (node < 1 || (size_t)node > n) { err = "vocabulary: word " + std::to_string(w) + " names node " + std::to_string(node) + ", outside 1 .. " + std::to_string(n); return false; }
    if (w < 0 || (size_t)w >= nw) { err = "vocabulary: word id " + std::to_string(w) + " outside 0 .. " + std::to_string((long long)nw - 1); return false; }
    if (seen[w]) { err = "vocabulary: word id " + std::to_string(w) + " given twice"; return false; }
    const int at = flatOf[node];
    if (f.childCount[at] != 0) { err = "vocabulary: word " + std::to_string(w) + " on inner node " + std::to_string(node); return false; }
    if (f.word[at] >= 0) { err = "vocabulary: node " + std::to_string(node) + " carries two words"; return false; }
    seen[w] = 1; f.word[at] = w; f.wordWeight[w] = v.weight[slot[node]];
  }
  for (size_t at = 1; at <= n; ++at)
    if (f.childCount[at] == 0 && f.word[at] < 0) { err = "vocabulary: leaf " + std::to_string(f.nodeOf[at]) + " without a word"; return false; }
  out = std::move(f);
  return true;
}

// the descent on the flat layout as the device walks it: the flat index of the leaf, 0 for a vocabulary without nodes
inline int ld_descend(const LdVocabFlat& f, const uint64_t q[4]) {
  int cur = 0;
  while (f.childCount[cur] > 0) {
    const int b = f.childBegin[cur];
    uint64_t best = ~0ull;
    for (int j = 0; j < f.childCount[cur]; ++j) {
      const uint64_t* d = &f.desc[4 * (size_t)(b + j)];
      const uint64_t dist = (uint64_t)(__builtin_popcountll(q[0] ^ d[0]) + __builtin_popcountll(q[1] ^ d[1]) +
                                       __builtin_popcountll(q[2] ^ d[2]) + __builtin_popcountll(q[3] ^ d[3]));
      const uint64_t key = dist << 32 | (uint64_t)j;
      if (key < best) best = key;
    }
    cur = b + (int)(best & 0xffffffffu);
  }
  return cur;
}

}  // namespace vpl
