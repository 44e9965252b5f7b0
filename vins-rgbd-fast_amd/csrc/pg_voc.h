// The vocabulary handle of vio_pg_voc_* (pg_bow.hip), shared with the batched database (pg_batch.hip), which borrows its device tree.
#pragma once
#include <stdint.h>

#include <utility>
#include <vector>

struct vio_pg_voc {
    int k = 0, L = 0, scoring = 0, weighting = 0, n_nodes = 0, n_words = 0, nentries = 0;
    // host copies (validation, info); the walk itself runs on the device
    std::vector<int> child_begin, children, node_word;
    std::vector<double> node_weight;
    // device tree
    int *d_child_begin = nullptr, *d_children = nullptr, *d_node_word = nullptr;
    double *d_node_weight = nullptr;
    uint64_t *d_node_desc = nullptr;
    // per-call device scratch (grown on demand)
    uint64_t *d_desc = nullptr;
    int *d_word = nullptr;
    double *d_w = nullptr;
    int cap = 0;
    std::vector<int> h_word;
    std::vector<double> h_w;
    // inverted file: word id -> (entry id, weight), rows in ascending entry order (TemplatedDatabase::add)
    std::vector<std::vector<std::pair<int, double>>> ifile;
    // query scratch
    std::vector<double> acc;
    std::vector<char> seen;
    std::vector<int> touched;
};
