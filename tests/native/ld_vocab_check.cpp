// Stand-alone check of csrc/ld_vocab.h (no GPU), built with the address and undefined-behaviour sanitizers by
// tests/test_ld_vocab.py: the file layout written and read back, every refusal of the vocabulary's validation, and the flat
// layout walked against a descent over a pointer tree built as loadBin builds it (TemplatedVocabulary.h:1509-1561, :1217-1258)
// for random irregular trees and random descriptors, ties included.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <random>
#include <string>
#include <vector>

#include "ld_vocab.h"

using namespace vpl;

static int failures = 0;
#define CHECK(cond, what)                                                      \
  do {                                                                         \
    if (!(cond)) { std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, what); ++failures; } \
  } while (0)

static uint64_t low_bits(int n) { return n >= 64 ? ~0ull : (1ull << n) - 1; }

// a random tree of n nodes: node i + 1 hangs under a random earlier node or the root (`bushy` favours few parents, so that some
// nodes get many children); leaves get the words in a random order; the records are shuffled when asked
static LdVocabRaw random_tree(std::mt19937_64& rng, int n, bool shuffle, int n_bits) {
  LdVocabRaw v;
  v.k = 10; v.L = 6; v.scoring = 0; v.weighting = (int)(rng() % 4);
  std::vector<int> parent(n + 1, 0), depth(n + 1, 0), kids(n + 1, 0);
  for (int id = 1; id <= n; ++id) {
    int p;
    do { p = (rng() % 3 == 0) ? (int)(rng() % (id < 4 ? id : 4)) : (int)(rng() % id); } while (depth[p] + 1 > LD_MAX_DEPTH);
    parent[id] = p; depth[id] = depth[p] + 1; kids[p]++;
  }
  std::vector<int> order(n);
  for (int i = 0; i < n; ++i) order[i] = i + 1;
  if (shuffle) std::shuffle(order.begin(), order.end(), rng);
  for (int id : order) {
    v.nodeId.push_back(id); v.parentId.push_back(parent[id]);
    v.weight.push_back((double)(rng() % 1000) / 64.0);
    // few distinct bits: equal descriptors among siblings and equal distances are common
    for (int q = 0; q < 4; ++q) v.desc.push_back(rng() & rng() & low_bits(n_bits) & (q == 0 ? ~0ull : 0x3ull));
  }
  std::vector<int> leaves;
  for (int id = 1; id <= n; ++id) if (!kids[id]) leaves.push_back(id);
  std::shuffle(leaves.begin(), leaves.end(), rng);
  for (size_t w = 0; w < leaves.size(); ++w) { v.wordNode.push_back(leaves[w]); v.wordId.push_back((int)w); }
  return v;
}

struct PNode { std::vector<int> children; uint64_t d[4] = {0, 0, 0, 0}; int word = -1; double weight = 0; };

static int pointer_descent(const std::vector<PNode>& nodes, const uint64_t* q, int* leaf) {
  int cur = 0;
  if (nodes[0].children.empty()) { *leaf = 0; return -1; }
  do {
    const std::vector<int>& c = nodes[cur].children;
    cur = c[0];
    int best = 0;
    for (int w = 0; w < 4; ++w) best += __builtin_popcountll(q[w] ^ nodes[cur].d[w]);
    for (size_t i = 1; i < c.size(); ++i) {
      int dist = 0;
      for (int w = 0; w < 4; ++w) dist += __builtin_popcountll(q[w] ^ nodes[c[i]].d[w]);
      if (dist < best) { best = dist; cur = c[i]; }
    }
  } while (!nodes[cur].children.empty());
  *leaf = cur;
  return nodes[cur].word;
}

static void check_descent(std::mt19937_64& rng, int n, bool shuffle, int n_bits) {
  const LdVocabRaw v = random_tree(rng, n, shuffle, n_bits);
  LdVocabFlat f;
  std::string err;
  CHECK(ld_flatten(v, f, err), err.c_str());
  if (f.nFlat != n + 1) { CHECK(false, "flat size"); return; }
  std::vector<PNode> nodes(n + 1);
  for (size_t i = 0; i < v.nodeId.size(); ++i) {
    PNode& p = nodes[v.nodeId[i]];
    p.weight = v.weight[i];
    for (int w = 0; w < 4; ++w) p.d[w] = v.desc[4 * i + w];
    nodes[v.parentId[i]].children.push_back(v.nodeId[i]);
  }
  for (size_t i = 0; i < v.wordId.size(); ++i) nodes[v.wordNode[i]].word = v.wordId[i];
  // the layout itself: every run of children is the parent's list in file order
  for (int at = 0; at < f.nFlat; ++at) {
    const PNode& p = nodes[f.nodeOf[at]];
    CHECK(f.childCount[at] == (int)p.children.size(), "child count");
    for (int j = 0; j < f.childCount[at] && j < (int)p.children.size(); ++j)
      CHECK(f.childBegin[at] + j < f.nFlat && f.nodeOf[f.childBegin[at] + j] == p.children[j], "children not in file order");
    CHECK(f.word[at] == (at ? p.word : -1) || (at == 0 && n == 0), "word of a node");
  }
  int ties = 0;
  for (int t = 0; t < 400; ++t) {
    uint64_t q[4];
    for (int w = 0; w < 4; ++w) q[w] = rng() & low_bits(n_bits) & (w == 0 ? ~0ull : 0x3ull);
    int leaf = 0;
    const int want = pointer_descent(nodes, q, &leaf);
    const int at = ld_descend(f, q);
    CHECK(f.nodeOf[at] == leaf, "descent ends at another leaf");
    CHECK((n == 0 && want == -1) || f.word[at] == want, "descent gives another word");
    if (want >= 0) CHECK(f.wordWeight[want] == nodes[leaf].weight, "weight of the word");
    // was there a tie on the way?  (count, to know the inputs do what they are for)
    int cur = 0;
    while (!nodes[cur].children.empty()) {
      int best = 1 << 30, nbest = 0, arg = -1;
      for (int c : nodes[cur].children) {
        int dist = 0;
        for (int w = 0; w < 4; ++w) dist += __builtin_popcountll(q[w] ^ nodes[c].d[w]);
        if (dist < best) { best = dist; nbest = 1; arg = c; } else if (dist == best) ++nbest;
      }
      ties += nbest > 1;
      cur = arg;
    }
  }
  if (n >= 50 && n_bits <= 8) CHECK(ties > 0, "no tie met on a tree made for ties");
}

static LdVocabRaw small() {   // root -> 1, 2; 1 -> 3, 4; words on 2, 3, 4
  LdVocabRaw v;
  v.k = 2; v.L = 2;
  v.nodeId = {1, 2, 3, 4}; v.parentId = {0, 0, 1, 1}; v.weight = {0, 1.5, 2.5, 3.5};
  v.desc.assign(16, 0);
  for (int i = 0; i < 4; ++i) v.desc[4 * i] = 0x11ull * (i + 1);
  v.wordNode = {2, 3, 4}; v.wordId = {0, 1, 2};
  return v;
}

static void refused(const LdVocabRaw& v, const char* expect) {
  LdVocabFlat f;
  f.nFlat = 777;   // must stay
  std::string err;
  const bool ok = ld_flatten(v, f, err);
  CHECK(!ok, expect);
  CHECK(err.find(expect) != std::string::npos, (std::string("reason '") + err + "' does not say '" + expect + "'").c_str());
  CHECK(f.nFlat == 777, "a refused vocabulary changed the output");
}

int main(int argc, char** argv) {
  const std::string dir = argc > 1 ? argv[1] : ".";
  std::mt19937_64 rng(12345);
  std::string err;
  // ---- the file layout, written and read back ----
  for (int n : {0, 1, 7, 300}) {
    const LdVocabRaw v = random_tree(rng, n, true, 64);
    const std::string path = dir + "/voc_" + std::to_string(n) + ".bin";
    CHECK(ld_write_file(path.c_str(), v, err), err.c_str());
    FILE* fp = std::fopen(path.c_str(), "rb");
    CHECK(fp != nullptr, "file not there");
    if (fp) { std::fseek(fp, 0, SEEK_END); CHECK(std::ftell(fp) == 24 + 48L * n + 8L * (long)v.wordId.size(), "file length"); std::fclose(fp); }
    LdVocabRaw r;
    CHECK(ld_read_file(path.c_str(), r, err), err.c_str());
    CHECK(r.k == v.k && r.L == v.L && r.scoring == v.scoring && r.weighting == v.weighting, "header");
    CHECK(r.nodeId == v.nodeId && r.parentId == v.parentId && r.weight == v.weight && r.desc == v.desc, "nodes");
    CHECK(r.wordNode == v.wordNode && r.wordId == v.wordId, "words");
    if (n == 300) {   // truncated: one byte short, inside the nodes, inside the header
      for (long cut : {24 + 48L * n + 8L * (long)v.wordId.size() - 1, 24 + 48L * 100 + 5, 23L, 0L}) {
        std::vector<unsigned char> all(cut);
        FILE* a = std::fopen(path.c_str(), "rb");
        CHECK(a && (cut == 0 || std::fread(all.data(), 1, cut, a) == (size_t)cut), "reread");
        if (a) std::fclose(a);
        const std::string tp = dir + "/voc_cut.bin";
        FILE* b = std::fopen(tp.c_str(), "wb");
        if (b) { if (cut) std::fwrite(all.data(), 1, cut, b); std::fclose(b); }
        LdVocabRaw t;
        t.k = 99;
        err.clear();
        CHECK(!ld_read_file(tp.c_str(), t, err) && err.find("truncated") != std::string::npos, "a truncated file was read");
        CHECK(t.k == 99 && t.nodeId.empty(), "a truncated file changed the output");
      }
    }
  }
  {   // a header that promises far more than the file holds sizes no allocation
    const std::string path = dir + "/voc_liar.bin";
    FILE* b = std::fopen(path.c_str(), "wb");
    const int32_t hdr[6] = {10, 6, 0, 0, 0x7fffffff, 0x7fffffff};
    if (b) { std::fwrite(hdr, 4, 6, b); std::fclose(b); }
    LdVocabRaw t;
    CHECK(!ld_read_file(path.c_str(), t, err) && err.find("truncated") != std::string::npos, "liar header");
    CHECK(!ld_read_file((dir + "/not_there.bin").c_str(), t, err), "missing file");
  }
  // ---- refusals ----
  {
    LdVocabFlat f;
    CHECK(ld_flatten(small(), f, err) && f.nFlat == 5 && f.nWords == 3 && f.depth == 2, "the small vocabulary itself");
    LdVocabRaw v;
    v = small(); v.nodeId[2] = 5; refused(v, "outside 1 ..");
    v = small(); v.nodeId[2] = 0; refused(v, "outside 1 ..");
    v = small(); v.nodeId[2] = 2; refused(v, "given twice");
    v = small(); v.parentId[3] = 9; refused(v, "is not a node");
    v = small(); v.parentId[3] = -1; refused(v, "is not a node");
    v = small(); v.parentId[0] = 3; refused(v, "cycle");                // 1 -> 3 -> 1
    v = small(); v.parentId[3] = 4; refused(v, "cycle");                // its own parent
    v = small(); v.wordNode.pop_back(); v.wordId.pop_back(); refused(v, "without a word");
    v = small(); v.wordNode[0] = 1; refused(v, "inner node");
    v = small(); v.wordNode[0] = 3; refused(v, "two words");
    v = small(); v.wordNode[0] = 7; refused(v, "names node");
    v = small(); v.wordId[0] = 3; refused(v, "outside 0 ..");
    v = small(); v.wordId[0] = -1; refused(v, "outside 0 ..");
    v = small(); v.wordId[0] = 1; refused(v, "given twice");
    for (int s = 1; s <= 5; ++s) { v = small(); v.scoring = s; refused(v, "L1_NORM"); }
    v = small(); v.weighting = 4; refused(v, "weighting");
    v = small(); v.weight.pop_back(); refused(v, "different lengths");
    // a chain of LD_MAX_DEPTH nodes stands, one more is refused
    for (int n : {LD_MAX_DEPTH, LD_MAX_DEPTH + 1}) {
      LdVocabRaw c;
      for (int i = 1; i <= n; ++i) { c.nodeId.push_back(i); c.parentId.push_back(i - 1); c.weight.push_back(1.0); }
      c.desc.assign(4 * n, 0); c.wordNode = {n}; c.wordId = {0};
      if (n == LD_MAX_DEPTH) CHECK(ld_flatten(c, f, err) && f.depth == LD_MAX_DEPTH, "a chain of the allowed depth"); else refused(c, "deeper than");
    }
    // all four weightings stand; the empty vocabulary stands and its descent stays at the root
    for (int w = 0; w < 4; ++w) { v = small(); v.weighting = w; CHECK(ld_flatten(v, f, err) && f.weighting == w, "weighting"); }
    LdVocabRaw e;
    CHECK(ld_flatten(e, f, err) && f.nFlat == 1 && f.nWords == 0 && f.childCount[0] == 0, "the empty vocabulary");
    const uint64_t q[4] = {1, 2, 3, 4};
    CHECK(ld_descend(f, q) == 0, "descent on the empty vocabulary");
  }
  // ---- the flat layout against the pointer tree ----
  for (int rep = 0; rep < 6; ++rep) {
    check_descent(rng, 0, false, 64);
    check_descent(rng, 1, false, 64);
    check_descent(rng, 5 + rep, true, 64);
    check_descent(rng, 60, true, 6);       // few bits: equal descriptors and equal distances
    check_descent(rng, 200, rep & 1, 8);
    check_descent(rng, 1500, true, 64);
  }
  if (failures) { std::printf("%d checks failed\n", failures); return 1; }
  std::printf("ld vocab ok\n");
  return 0;
}
