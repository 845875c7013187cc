// safetensors_main.cpp -- drives the host-only checkpoint code (csrc/safetensors_reader.cpp, csrc/ckpt_keys.cpp; no HIP headers) under
// AddressSanitizer + UBSan as a plain program (tests/test_safetensors_cpu.py builds and runs it):
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all tests/san/safetensors_main.cpp csrc/safetensors_reader.cpp csrc/ckpt_keys.cpp
//   ./a.out <well-formed.safetensors> <tests/golden/sd14_ckpt_keys.txt> <scratch directory>
// 1. the key rules over every fixture line, and over mangled names (every prefix, every single-character change of a few names);
// 2. the reader over the well-formed file, over every truncation of its header and over byte flips at every header position -- each case parsed from a
//    heap copy of exactly the bytes it may read, so that one byte too far is an ASan report -- and over truncated copies of the whole file;
// 3. the default schedule.
// A refusal (sdmi::Error) is a pass; so is an accepted mutation (many flips only rename a key).  Prints "ok: <cases> cases" and exits 0.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <fstream>
#include <iostream>
#include <memory>
#include <sstream>
#include <string>
#include <vector>

#include "../../stable_diffusion_burn_amd/csrc/ckpt_keys.hpp"
#include "../../stable_diffusion_burn_amd/csrc/error.hpp"
#include "../../stable_diffusion_burn_amd/csrc/safetensors_reader.hpp"

static long g_cases = 0, g_refused = 0;

static int fail(const std::string& what) {
    std::cerr << "FAIL: " << what << "\n";
    return 1;
}

// parse `n` header bytes from an exact-size heap block
static void parse_exact(const unsigned char* bytes, size_t n, size_t data_bytes) {
    std::unique_ptr<unsigned char[]> copy(new unsigned char[n ? n : 1]);
    if (n) std::memcpy(copy.get(), bytes, n);
    std::vector<sdmi::StTensor> out;
    ++g_cases;
    try {
        sdmi::SafetensorsFile::parse_header(copy.get(), n, data_bytes, nullptr, 0, &out);
        for (const auto& t : out)
            if (t.file_offset + t.nbytes > data_bytes) throw std::logic_error("accepted a tensor outside the data section: " + t.key);
    } catch (const sdmi::Error& e) {
        if (e.status != SDMI_ERR_WEIGHTS || !*e.what()) throw std::logic_error("a malformed header must be SDMI_ERR_WEIGHTS with a message");
        ++g_refused;
    }
}

int main(int argc, char** argv) {
    if (argc != 4) return fail("usage: safetensors_main <file.safetensors> <sd14_ckpt_keys.txt> <scratch dir>");
    const std::string file = argv[1], fixture = argv[2], scratch = argv[3];
    try {
        // ---- 1. key rules ----------------------------------------------------------------------------------------------------------
        std::ifstream fx(fixture);
        if (!fx) return fail("cannot open " + fixture);
        std::string line;
        std::vector<std::string> names;
        while (std::getline(fx, line)) {
            std::istringstream ls(line);
            std::string dump, key, shape, flag;
            std::getline(ls, dump, '\t'); std::getline(ls, key, '\t'); std::getline(ls, shape, '\t'); std::getline(ls, flag, '\t');
            std::string got;
            bool tr = false;
            ++g_cases;
            if (!sdmi::checkpoint_key(dump, &got, &tr) || got != key || tr != (flag == "T")) return fail("checkpoint_key('" + dump + "') = '" + got + "', fixture: '" + key + "' " + flag);
            names.push_back(dump);
        }
        if (names.size() < 1000) return fail("fixture too short");
        for (size_t i = 0; i < names.size(); i += 97) {
            const std::string& n = names[i];
            std::string got;
            bool tr;
            for (size_t cut = 0; cut <= n.size(); ++cut) { ++g_cases; (void)sdmi::checkpoint_key(n.substr(0, cut), &got, &tr); (void)sdmi::checkpoint_key(n.substr(cut), nullptr, nullptr); }
            for (size_t pos = 0; pos < n.size(); ++pos)
                for (char c : {'/', '0', '9', '\0', 'x', (char)0xff}) { std::string m = n; m[pos] = c; ++g_cases; (void)sdmi::checkpoint_key(m, &got, &tr); }
        }
        for (const char* meta : {"n_steps", "unet/norm_out/eps", "unet/norm_out/n_group", "clip/n_layer", "autoencoder/decoder/n_block", "", "/", "unet/", "unet//weight"}) {
            ++g_cases;
            if (sdmi::checkpoint_key(meta, nullptr, nullptr)) return fail(std::string("accepted '") + meta + "'");
        }

        // ---- 2. the reader ---------------------------------------------------------------------------------------------------------
        std::ifstream in(file, std::ios::binary);
        if (!in) return fail("cannot open " + file);
        std::vector<unsigned char> bytes((std::istreambuf_iterator<char>(in)), std::istreambuf_iterator<char>());
        if (bytes.size() < 8) return fail("input too short");
        uint64_t hlen = 0;
        for (int i = 7; i >= 0; --i) hlen = (hlen << 8) | bytes[(size_t)i];
        if (hlen > bytes.size() - 8) return fail("input is not well formed");
        const unsigned char* header = bytes.data() + 8;
        const size_t data_bytes = bytes.size() - 8 - (size_t)hlen;
        size_t n_tensors = 0;
        {
            sdmi::SafetensorsFile f(file);
            n_tensors = f.tensors().size();
            unsigned long long sum = 0;
            for (const auto& t : f.tensors()) {   // every byte the index points at is inside the mapping
                for (size_t i = 0; i < t.nbytes; ++i) sum += t.data[i];
                if (f.find(t.key) != &t) return fail("find('" + t.key + "')");
            }
            if (!n_tensors) return fail("no tensors in the well-formed file");
            std::printf("well-formed: %zu tensors, byte sum %llu\n", n_tensors, sum);
        }
        const long before = g_refused;
        parse_exact(header, (size_t)hlen, data_bytes);
        if (g_refused != before) return fail("the well-formed header was refused");
        for (size_t cut = 0; cut < (size_t)hlen; ++cut) parse_exact(header, cut, data_bytes);
        {
            // every cut that ends inside the object must be refused (only trailing padding may go)
            size_t end = (size_t)hlen;
            while (end && header[end - 1] == ' ') --end;
            const long r0 = g_refused;
            for (size_t cut = 0; cut < end; ++cut) parse_exact(header, cut, data_bytes);
            if (g_refused - r0 != (long)end) return fail("a truncated header was accepted");
        }
        std::vector<unsigned char> h(header, header + hlen);
        for (size_t pos = 0; pos < h.size(); ++pos) {
            const unsigned char keep = h[pos];
            for (unsigned char v : {(unsigned char)(keep ^ 1), (unsigned char)(keep ^ 0x80), (unsigned char)'"', (unsigned char)'\\', (unsigned char)'{', (unsigned char)'}',
                                    (unsigned char)'[', (unsigned char)',', (unsigned char)'-', (unsigned char)'9', (unsigned char)'u', (unsigned char)0}) {
                h[pos] = v;
                parse_exact(h.data(), h.size(), data_bytes);
            }
            h[pos] = keep;
        }
        parse_exact(header, (size_t)hlen, data_bytes ? data_bytes - 1 : 0);   // a data section one byte short
        parse_exact(header, (size_t)hlen, 0);
        for (size_t keep : {(size_t)0, (size_t)4, (size_t)8, (size_t)(8 + hlen / 2), (size_t)(8 + hlen), bytes.size() - 1}) {
            const std::string p = scratch + "/cut_" + std::to_string(keep) + ".safetensors";
            { std::ofstream o(p, std::ios::binary); o.write(reinterpret_cast<const char*>(bytes.data()), (std::streamsize)keep); }
            ++g_cases;
            try {
                sdmi::SafetensorsFile f(p);
                if (data_bytes && keep < bytes.size() && !f.tensors().empty() && keep >= 8 + hlen) {
                    size_t total = 0;
                    for (const auto& t : f.tensors()) total += t.nbytes;
                    if (total > keep - 8 - hlen) return fail("a file truncated to " + std::to_string(keep) + " bytes was accepted");
                }
            } catch (const sdmi::Error& e) {
                if (e.status != SDMI_ERR_WEIGHTS && e.status != SDMI_ERR_IO) return fail("unexpected status for a truncated file");
                ++g_refused;
            }
        }
        ++g_cases;
        try { sdmi::SafetensorsFile f(scratch + "/does_not_exist.safetensors"); return fail("opened a missing file"); }
        catch (const sdmi::Error& e) { if (e.status != SDMI_ERR_IO) return fail("a missing file must be SDMI_ERR_IO"); ++g_refused; }

        // ---- 3. the default schedule -----------------------------------------------------------------------------------------------
        std::vector<float> a(1000);
        sdmi::default_alphas_cumprod(a.data(), 1000);
        ++g_cases;
        if (!(std::fabs(a[0] - 0.99915f) < 1e-6f) || !(a[999] > 0.0046f && a[999] < 0.0047f)) return fail("default_alphas_cumprod");
        for (int i = 1; i < 1000; ++i)
            if (!(a[(size_t)i] < a[(size_t)i - 1])) return fail("default_alphas_cumprod is not decreasing");
        float one = 0;
        sdmi::default_alphas_cumprod(&one, 1);
    } catch (const std::exception& e) {
        return fail(std::string("exception: ") + e.what());
    }
    std::printf("ok: %ld cases, %ld refused\n", g_cases, g_refused);
    return 0;
}
