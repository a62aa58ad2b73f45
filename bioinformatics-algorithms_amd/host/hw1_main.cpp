// hw1_main.cpp -- `hw1`-compatible command line over the MI355X engine (libpwalign.so).
//
// Same surface as the reference program multiple_pattern_matching/multiple_pattern_matching.cpp (main):
//   hw1_amd -r <reference.fasta> -p <patterns.fasta> -o <output_prefix> [-d]
// same argument handling, stderr texts, exit codes and output bytes (<prefix>.txt, and <prefix>.dot with -d).
// The reference builds one Ukkonen suffix tree over all references joined by terminators and walks it per pattern;
// here the same text goes to the device as a suffix array (pwa_sa_create), every pattern is searched at once
// (pwa_sa_find for the sizes, pwa_sa_occurrences for the (header, position) keys in output order), and the host
// only formats.  -d rebuilds the tree's DOT text from the suffix array on the host (hw1_host.h).
#include <algorithm>
#include <chrono>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <iostream>
#include <numeric>
#include <string>
#include <vector>

#include "../../include/pwalign.h"
#include "hw1_host.h"

namespace {

struct Records {   // owns an hw1_records
    hw1_records* r;
    explicit Records(const std::string& path) : r(hw1_read_sequences(path.c_str(), nullptr)) {}
    ~Records() { hw1_records_free(r); }
    uint32_t size() const { return hw1_records_count(r); }
    std::string header(uint32_t i) const {
        uint64_t n = 0;
        const char* p = hw1_records_header(r, i, &n);
        return std::string(p, n);
    }
    std::string seq(uint32_t i) const {
        uint64_t n = 0;
        const char* p = hw1_records_sequence(r, i, &n);
        return std::string(p, n);
    }
};

bool g_debug = false;
auto g_t = std::chrono::steady_clock::now();
void phase(const char* what) {
    if (!g_debug) return;
    const auto now = std::chrono::steady_clock::now();
    std::fprintf(stderr, "[hw1_amd] %-22s %10.3f ms\n", what, std::chrono::duration<double, std::milli>(now - g_t).count());
    g_t = now;
}

int gpu_error(const char* what, int rc, pwa_ctx* ctx) {
    std::cerr << "Error: " << what << " failed: " << pwa_strerror(rc);
    if (ctx) std::cerr << " (" << pwa_last_error(ctx) << ")";
    std::cerr << " (no CPU fallback exists)" << std::endl;
    return 2;
}

}  // namespace

int main(int argc, char** argv) {
    g_debug = std::getenv("PWA_DEBUG") != nullptr;
    std::string ref_file, pat_file, prefix;
    bool dot = false;
    for (int i = 1; i < argc; ++i) {   // unknown arguments are ignored, as in the reference
        const std::string arg = argv[i];
        if (arg == "-r" && i + 1 < argc) ref_file = argv[++i];
        else if (arg == "-p" && i + 1 < argc) pat_file = argv[++i];
        else if (arg == "-o" && i + 1 < argc) prefix = argv[++i];
        else if (arg == "-d") dot = true;
    }
    if (ref_file.empty() || pat_file.empty() || prefix.empty()) {
        std::cerr << "Usage: " << argv[0] << " -r <reference.fasta> -p <patterns.fasta> -o <output_prefix> [-d]" << std::endl;
        return 1;
    }
    const Records refs(ref_file), pats(pat_file);
    phase("read FASTA");

    // T = each reference followed by its terminator
    const uint32_t n_ref = refs.size(), n_pat = pats.size();
    std::string text;
    std::vector<uint32_t> ref_start(n_ref + 1, 0);
    std::vector<std::string> names(n_ref);
    for (uint32_t r = 0; r < n_ref; ++r) {
        if (text.size() >= (1ull << 31)) break;
        ref_start[r] = (uint32_t)text.size();
        text += refs.seq(r);
        text.push_back((char)hw1_terminator(n_ref, r));
        names[r] = refs.header(r);
    }
    if (text.size() >= (1ull << 31)) {
        std::cerr << "Error: the references and their terminators make " << text.size()
                  << " bytes; positions are int32, so at most 2147483647" << std::endl;
        return 1;
    }
    ref_start[n_ref] = (uint32_t)text.size();
    // header ranks in std::string order; references that share a header share a rank (one entry per header)
    std::vector<uint32_t> by_name(n_ref), header_rank(n_ref);
    std::iota(by_name.begin(), by_name.end(), 0u);
    std::stable_sort(by_name.begin(), by_name.end(), [&](uint32_t a, uint32_t b) { return names[a] < names[b]; });
    std::vector<const std::string*> rank_name;
    for (uint32_t k = 0; k < n_ref; ++k) {
        const uint32_t r = by_name[k];
        if (k == 0 || names[r] != *rank_name.back()) rank_name.push_back(&names[r]);
        header_rank[r] = (uint32_t)rank_name.size() - 1;
    }
    std::string pblob;
    std::vector<uint64_t> poff(n_pat + 1, 0);
    std::vector<std::string> pnames(n_pat);
    for (uint32_t k = 0; k < n_pat; ++k) {
        poff[k] = pblob.size();
        pblob += pats.seq(k);
        pnames[k] = pats.header(k);
    }
    poff[n_pat] = pblob.size();
    phase("text + patterns");

    const std::string txt_path = prefix + ".txt";
    FILE* out = std::fopen(txt_path.c_str(), "wb");
    if (!out) {
        std::cerr << "Cannot open output file: " << txt_path << std::endl;
        return 1;
    }

    // the device is needed for hits (a text and patterns) and for -d over a non-empty text
    const bool need_hits = !text.empty() && n_pat > 0, need_sa = dot && !text.empty();
    std::vector<uint64_t> occ_off(n_pat + 1, 0), occ;
    std::vector<uint32_t> sa;
    if (need_hits || need_sa) {
        struct Device {   // released on every way out
            pwa_ctx* ctx = nullptr;
            pwa_sa_index* ix = nullptr;
            ~Device() {
                pwa_sa_destroy(ix);
                pwa_ctx_destroy(ctx);
            }
        } dev;
        int rc = pwa_ctx_create(0, &dev.ctx);
        if (rc != PWA_OK) return gpu_error("opening the MI355X device", rc, nullptr);
        phase("device context");
        rc = pwa_sa_create(dev.ctx, reinterpret_cast<const uint8_t*>(text.data()), text.size(), &dev.ix);
        if (rc != PWA_OK) return gpu_error("pwa_sa_create", rc, dev.ctx);
        phase("suffix array");
        const uint8_t* pb = reinterpret_cast<const uint8_t*>(pblob.data());
        if (need_hits) {
            std::vector<uint32_t> cnt(n_pat);
            rc = pwa_sa_find(dev.ix, pb, poff.data(), n_pat, cnt.data());
            if (rc != PWA_OK) return gpu_error("pwa_sa_find", rc, dev.ctx);
            occ.resize(std::accumulate(cnt.begin(), cnt.end(), uint64_t(0)));   // raw hits bound the kept ones
            phase("search (sizes)");
            uint64_t needed = 0;
            rc = pwa_sa_occurrences(dev.ix, pb, poff.data(), n_pat, ref_start.data(), n_ref, header_rank.data(), occ_off.data(), occ.data(),
                                    occ.size(), &needed);
            if (rc != PWA_OK) return gpu_error("pwa_sa_occurrences", rc, dev.ctx);
            phase("occurrences");
        }
        if (need_sa) {
            sa.resize(text.size());
            rc = pwa_sa_fetch(dev.ix, sa.data());
            if (rc != PWA_OK) return gpu_error("pwa_sa_fetch", rc, dev.ctx);
        }
        if (g_debug) {
            uint32_t rounds = 0;
            float build_ms = 0, search_ms = 0;
            pwa_sa_last_stats(dev.ix, &rounds, &build_ms, &search_ms);
            std::fprintf(stderr, "[hw1_amd] text %zu bytes, %u references, %u patterns, %llu occurrences: SA %u rounds, device %.3f ms; "
                                 "occurrences call %.3f ms\n", text.size(), n_ref, n_pat, (unsigned long long)occ_off[n_pat], rounds, build_ms, search_ms);
        }
    }

    // "(name) - header:pos,pos, header:pos" per pattern, headers in std::string order
    std::vector<char> buf(1 << 20);
    std::setvbuf(out, buf.data(), _IOFBF, buf.size());
    char num[24];
    for (uint32_t k = 0; k < n_pat; ++k) {
        std::fputc('(', out);
        std::fwrite(pnames[k].data(), 1, pnames[k].size(), out);
        std::fputs(") - ", out);
        uint64_t last_rank = ~0ull;
        for (uint64_t e = occ_off[k]; e < occ_off[k + 1]; ++e) {
            const uint64_t rank = occ[e] >> 32;
            if (rank != last_rank) {
                if (last_rank != ~0ull) std::fputs(", ", out);
                std::fwrite(rank_name[rank]->data(), 1, rank_name[rank]->size(), out);
                std::fputc(':', out);
                last_rank = rank;
            } else {
                std::fputc(',', out);
            }
            const int len = std::snprintf(num, sizeof num, "%u", (uint32_t)occ[e]);
            std::fwrite(num, 1, (size_t)len, out);
        }
        std::fputc('\n', out);
    }
    std::fclose(out);
    phase("write .txt");
    if (dot) {
        std::vector<const char*> hp(n_ref);
        std::vector<uint64_t> hl(n_ref);
        for (uint32_t r = 0; r < n_ref; ++r) {
            hp[r] = names[r].data();
            hl[r] = names[r].size();
        }
        (void)hw1_write_dot((prefix + ".dot").c_str(), reinterpret_cast<const uint8_t*>(text.data()), (uint32_t)text.size(), sa.data(), n_ref,
                            ref_start.data(), hp.data(), hl.data());
        phase("write .dot");
    }
    return 0;
}
