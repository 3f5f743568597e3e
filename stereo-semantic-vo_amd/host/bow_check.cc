// bow_check.cc - one frame through a vocabulary (svo_bow_create_from_text + svo_bow_transform), from the command line.
// usage: bow_check voc.txt desc.bin [levelsup, default 0]
// desc.bin: n x 32 bytes, one descriptor after the other (n <= 2048).
// stdout: "# k L nodes words weighting"; "n_features n_words n_pairs"; the features' words in one line (-1: a stop word); then
// "word value" (%.17g) per entry of the BowVector and "node feature" per pair of the FeatureVector.
#include <cstdio>
#include <cstdlib>
#include <iostream>
#include <vector>

#include "../../include/svo.h"

int main(int argc, char** argv) {
  if (argc < 3 || argc > 4) {
    std::cerr << "Usage: ./bow_check voc.txt desc.bin [levelsup]" << std::endl;
    return 1;
  }
  FILE* in = fopen(argv[2], "rb");
  if (!in) { std::cerr << argv[2] << ": cannot open" << std::endl; return 1; }
  std::vector<uint8_t> desc;
  uint8_t buf[4096];
  size_t got;
  while ((got = fread(buf, 1, sizeof buf, in)) > 0) desc.insert(desc.end(), buf, buf + got);
  fclose(in);
  if (desc.size() % 32 || desc.size() / 32 > 2048) { std::cerr << argv[2] << ": not n x 32 bytes with n <= 2048" << std::endl; return 1; }
  const int n = (int)(desc.size() / 32), levelsup = argc > 3 ? atoi(argv[3]) : 0;
  svo_bow* bow = nullptr;
  if (svo_bow_create_from_text(0, argv[1], n > 0 ? n : 1, 1, &bow) != SVO_OK) {
    std::cerr << "svo_bow_create_from_text: " << svo_bow_last_error(nullptr) << std::endl;
    return 1;
  }
  int k, L, nodes, nwords, weighting;
  svo_bow_describe(bow, &k, &L, &nodes, &nwords, &weighting);
  std::vector<int32_t> words((size_t)n + 1);
  std::vector<svo_bow_entry> vec((size_t)n + 1);
  std::vector<svo_bow_feature> fv((size_t)n + 1);
  int32_t nv = 0, nf = 0;
  if (svo_bow_transform(bow, desc.data(), n, levelsup, words.data(), vec.data(), &nv, fv.data(), &nf) != SVO_OK) {
    std::cerr << "svo_bow_transform: " << svo_bow_last_error(bow) << std::endl;
    svo_bow_destroy(bow);
    return 1;
  }
  svo_bow_destroy(bow);
  printf("# %d %d %d %d %d\n%d %d %d\n", k, L, nodes, nwords, weighting, n, nv, nf);
  for (int i = 0; i < n; ++i) printf("%d%s", words[i], i + 1 == n ? "" : " ");
  printf("\n");
  for (int i = 0; i < nv; ++i) printf("%u %.17g\n", vec[i].word, vec[i].value);
  for (int i = 0; i < nf; ++i) printf("%u %u\n", fv[i].node, fv[i].feature);
  return 0;
}
