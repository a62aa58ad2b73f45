// hw1_host.cpp -- readSequences, the terminator list and printDot of the hw1 reference, for hw1_amd (hw1_host.h).
#include "hw1_host.h"

#include <algorithm>
#include <cstdio>
#include <fstream>
#include <iostream>
#include <new>
#include <string>
#include <utility>
#include <vector>

struct hw1_records {
    std::vector<std::pair<std::string, std::string>> rec;   // (header, sequence)
};

extern "C" {

hw1_records* hw1_read_sequences(const char* path, int* opened) {
    hw1_records* out = new (std::nothrow) hw1_records();
    if (!out) return nullptr;
    std::ifstream file(path);
    if (opened) *opened = file ? 1 : 0;
    if (!file) {
        std::cerr << "Cannot open file: " << path << std::endl;
        return out;
    }
    std::string line, header, seq;
    while (std::getline(file, line)) {
        if (line.empty()) break;   // the first empty line ends the file, before trimming
        line.erase(line.find_last_not_of(" \t\r\n") + 1);
        line.erase(0, line.find_first_not_of(" \t\r\n"));
        if (!line.empty() && line[0] == '>') {
            if (!header.empty()) {
                out->rec.emplace_back(header, seq);
                seq.clear();
            }
            header = line.substr(1);
        } else {
            seq += line;
        }
    }
    if (!header.empty()) out->rec.emplace_back(header, seq);
    return out;
}

uint32_t hw1_records_count(const hw1_records* r) { return r ? (uint32_t)r->rec.size() : 0; }

const char* hw1_records_header(const hw1_records* r, uint32_t i, uint64_t* len) {
    if (len) *len = r->rec[i].first.size();
    return r->rec[i].first.data();
}

const char* hw1_records_sequence(const hw1_records* r, uint32_t i, uint64_t* len) {
    if (len) *len = r->rec[i].second.size();
    return r->rec[i].second.data();
}

void hw1_records_free(hw1_records* r) { delete r; }

int hw1_terminator(uint32_t n_refs, uint32_t i) {
    static const char kFew[] = "$#@%^&!";
    if (n_refs <= 7) return (uint8_t)kFew[i];
    static const std::vector<uint8_t> many = [] {
        std::vector<uint8_t> v;
        for (int c = 33; c < 127; ++c)
            if (c != 'A' && c != 'C' && c != 'G' && c != 'T') v.push_back((uint8_t)c);
        return v;
    }();
    return many[i % many.size()];
}

int hw1_write_dot(const char* path, const uint8_t* text, uint32_t n, const uint32_t* sa, uint32_t n_ref, const uint32_t* ref_start,
                  const char* const* headers, const uint64_t* header_len) try {
    FILE* f = std::fopen(path, "wb");
    if (!f) return -1;
    std::vector<char> buf(1 << 20);
    std::setvbuf(f, buf.data(), _IOFBF, buf.size());
    std::fputs("digraph suffix_tree {\n", f);
    if (n == 0) {   // the root alone is a leaf: suffix index |T| - 0 = 0, in no reference
        std::fputs("node0 [label=\"0\"];\n}\n", f);
        return std::fclose(f) == 0 ? 0 : -1;
    }
    // LCP[i] = common prefix of the suffixes at SA[i - 1] and SA[i] (Kasai)
    std::vector<uint32_t> lcp(n, 0);
    {
        std::vector<uint32_t> rank(n);
        for (uint32_t i = 0; i < n; ++i) rank[sa[i]] = i;
        uint32_t h = 0;
        for (uint32_t p = 0; p < n; ++p) {
            if (rank[p] == 0) {
                h = 0;
                continue;
            }
            const uint32_t q = sa[rank[p] - 1];
            while (p + h < n && q + h < n && text[p + h] == text[q + h]) ++h;
            lcp[rank[p]] = h;
            if (h) --h;
        }
    }
    // internal nodes other than the root: the LCP intervals (left end, string depth), in pre-order = by (left end, depth)
    struct Node {
        uint32_t lb, depth;
    };
    std::vector<Node> inner, st{{0, 0}};
    for (uint32_t i = 1; i <= n; ++i) {
        const uint32_t l = i < n ? lcp[i] : 0;
        uint32_t lb = i - 1;
        while (l < st.back().depth) {
            inner.push_back(st.back());
            lb = st.back().lb;
            st.pop_back();
        }
        if (l > st.back().depth) st.push_back({lb, l});
    }
    std::sort(inner.begin(), inner.end(), [](const Node& a, const Node& b) { return a.lb != b.lb ? a.lb < b.lb : a.depth < b.depth; });

    struct Open {
        uint64_t id;
        uint32_t lb, depth;
    };
    std::vector<Open> path{{0, 0, 0}};
    uint64_t next_id = 1;
    std::fputs("node0 [label=\"\"];\n", f);
    auto edge = [&](uint64_t from, uint64_t to, uint64_t b, uint64_t e) {
        std::fprintf(f, "node%llu -> node%llu [label=\"", (unsigned long long)from, (unsigned long long)to);
        std::fwrite(text + b, 1, e - b, f);
        std::fputs("\"];\n", f);
    };
    auto close_deeper = [&](uint32_t depth) {   // each child's edge line follows its whole subtree
        while (path.back().depth > depth) {
            const Open c = path.back();
            path.pop_back();
            edge(path.back().id, c.id, (uint64_t)sa[c.lb] + path.back().depth, (uint64_t)sa[c.lb] + c.depth);
        }
    };
    size_t q = 0;
    for (uint32_t i = 0; i < n; ++i) {
        if (i) close_deeper(lcp[i]);
        for (; q < inner.size() && inner[q].lb == i; ++q) {
            std::fprintf(f, "node%llu [label=\"\"];\n", (unsigned long long)next_id);
            path.push_back({next_id++, inner[q].lb, inner[q].depth});
        }
        const uint32_t p = sa[i];
        const uint32_t r = (uint32_t)(std::upper_bound(ref_start, ref_start + n_ref + 1, p) - ref_start) - 1;
        std::fprintf(f, "node%llu [label=\"", (unsigned long long)next_id);
        if (r < n_ref && p + 1 < ref_start[r + 1]) {
            std::fwrite(headers[r], 1, header_len[r], f);
            std::fprintf(f, ":%u:%u\"];\n", p - ref_start[r], p);
        } else {
            std::fprintf(f, "%u\"];\n", p);
        }
        edge(path.back().id, next_id, (uint64_t)p + path.back().depth, n);
        ++next_id;
    }
    close_deeper(0);
    std::fputs("}\n", f);
    return std::fclose(f) == 0 ? 0 : -1;
} catch (...) {
    return -1;
}

}  // extern "C"
