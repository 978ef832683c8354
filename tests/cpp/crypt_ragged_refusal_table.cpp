// crypt_ragged_refusal_table.cpp — the argument refusals of p252_{encrypt,decrypt}_ragged_device_into and of p252_encryption_tags, as a
// table in the format of api_refusals.cpp:
//   symbol <TAB> case <TAB> rc <TAB> p252_last_error
// Every refusal happens before the entry point binds its device, so a context that never saw a device (device = -1) reaches all of
// them with or without a GPU.  The control row must get past validation and fail at hipSetDevice(ctx->device) with P252_ERR_HIP;
// every other row varies the control one way.  The buffers are addresses 1 MiB apart that nothing dereferences: no row reaches a
// device.  (tests/test_crypt_ragged_cpu.py compares the lines with tests/golden/crypt_ragged_refusals.txt.)
#include "refusal_table.hpp"

using namespace refusal;

namespace {

// in / out: the message and the cipher side (encrypt), the cipher and the message side (decrypt); d_ok: decrypt only
struct Crypt {
    p252_ctx* ctx;
    uint64_t variant, d_tags, max_len, d_in, n_scalars, d_offsets, d_secrets, d_nonces, d_out, d_ok, n, d_n_bad;
};

int call(bool decrypt, const Crypt& a) {
    if (decrypt)
        return p252_decrypt_ragged_device_into(a.ctx, (int)a.variant, P(a.d_tags), a.max_len, P(a.d_in), a.n_scalars, P(a.d_offsets), P(a.d_secrets),
                                          P(a.d_nonces), P(a.d_out), P(a.d_ok), a.n, P(a.d_n_bad), nullptr);
    return p252_encrypt_ragged_device_into(a.ctx, (int)a.variant, P(a.d_tags), a.max_len, P(a.d_in), a.n_scalars, P(a.d_offsets), P(a.d_secrets),
                                      P(a.d_nonces), P(a.d_out), a.n, P(a.d_n_bad), nullptr);
}

struct In {
    const char* name;
    uint64_t Crypt::*at;
    uint64_t bytes;
};

}  // namespace

int main() {
    p252_ctx* ctx = new p252_ctx();  // device = -1: never bound
    for (bool decrypt : {false, true}) {
        const char* sym = decrypt ? "p252_decrypt_ragged_device_into" : "p252_encrypt_ragged_device_into";
        // 6 messages of at most 42 scalars, 100 scalars in all: 106 on the cipher side
        const Crypt good = {ctx, P252_CRYPT_STREAM, slot(0), 42, slot(1), 100, slot(2), slot(3), slot(4), slot(5), slot(6), 6, slot(7)};
        using Case = CaseOf<Crypt>;
        std::vector<Case> cases = {
            {"control", [](Crypt&) {}},
            {"ctx=NULL", [](Crypt& a) { a.ctx = nullptr; }},
            {"variant=DUPLEX", [](Crypt& a) { a.variant = P252_CRYPT_DUPLEX; }},
            {"variant=2", [](Crypt& a) { a.variant = 2; }},
            {"variant=-1", [](Crypt& a) { a.variant = (uint64_t)-1; }},
            {"n=0", [](Crypt& a) { a.n = 0; }},
            {"n=0,all=NULL", [ctx](Crypt& a) { a = Crypt{ctx, 0, 0, 1, 0, 0, 0, 0, 0, 0, 0, 0, 0}; }},
            {"n=0,max_len=0", [](Crypt& a) { a.n = 0, a.max_len = 0; }},
            {"max_len=0", [](Crypt& a) { a.max_len = 0; }},
            {"max_len=1", [](Crypt& a) { a.max_len = 1; }},
            {"max_len=cap", [](Crypt& a) { a.max_len = P252_CRYPT_RAGGED_MAX_LEN; }},
            {"max_len=cap+1", [](Crypt& a) { a.max_len = P252_CRYPT_RAGGED_MAX_LEN + 1; }},
            {"max_len=SIZE_MAX", [](Crypt& a) { a.max_len = MAXZ; }},
            {"n_scalars=0", [](Crypt& a) { a.n_scalars = 0; }},
            {"d_n_bad=NULL", [](Crypt& a) { a.d_n_bad = 0; }},
            {"n=SIZE_MAX/128", [](Crypt& a) { a.n = MAXZ / 128; }},
            {"n=SIZE_MAX", [](Crypt& a) { a.n = MAXZ; }},
            {"n_scalars=SIZE_MAX/64", [](Crypt& a) { a.n_scalars = MAXZ / 64; }},
            {"n_scalars=SIZE_MAX", [](Crypt& a) { a.n_scalars = MAXZ; }},
            {"n_scalars+n=SIZE_MAX/64", [](Crypt& a) { a.n_scalars = MAXZ / 64 - 6; }},
            {"n_scalars+n=SIZE_MAX/64-1", [](Crypt& a) { a.n_scalars = MAXZ / 64 - 7; }},
        };
        std::vector<BufOf<Crypt>> bufs = {{"d_tags", &Crypt::d_tags, 16},       {"d_in", &Crypt::d_in, 16},       {"d_offsets", &Crypt::d_offsets, 8},
                                          {"d_secrets", &Crypt::d_secrets, 16}, {"d_nonces", &Crypt::d_nonces, 16}, {"d_out", &Crypt::d_out, 16}};
        if (decrypt) bufs.push_back({"d_ok", &Crypt::d_ok, 1});
        for (const BufOf<Crypt>& b : bufs) {
            cases.push_back({std::string(b.name) + "=NULL", [b](Crypt& a) { a.*(b.at) = 0; }});
            if (b.align > 1) cases.push_back({std::string(b.name) + "+" + std::to_string(b.align / 2), [b](Crypt& a) { a.*(b.at) += b.align / 2; }});
        }
        cases.push_back({"d_n_bad+2", [](Crypt& a) { a.d_n_bad += 2; }});
        // every output against every input and every other output: inside the other's last 16 bytes, and just behind it
        const uint64_t msg = 100 * 32, cph = 106 * 32;
        const In ins[] = {{"d_tags", &Crypt::d_tags, 42 * 32},
                          {"d_in", &Crypt::d_in, decrypt ? cph : msg},
                          {"d_offsets", &Crypt::d_offsets, 7 * 8},
                          {"d_secrets", &Crypt::d_secrets, 6 * 64},
                          {"d_nonces", &Crypt::d_nonces, 6 * 32}};
        std::vector<In> outs = {{"d_out", &Crypt::d_out, decrypt ? msg : cph}};
        if (decrypt) outs.push_back({"d_ok", &Crypt::d_ok, 6});
        outs.push_back({"d_n_bad", &Crypt::d_n_bad, 4});
        for (size_t x = 0; x < outs.size(); ++x) {
            const In o = outs[x];
            auto add = [&](const In& i) {
                uint64_t Crypt::*in_at = i.at;
                const uint64_t last = (i.bytes - 1) & ~15ull, in_bytes = (i.bytes + 15) & ~15ull;
                cases.push_back({std::string(o.name) + "=" + i.name + "+last", [o, in_at, last](Crypt& a) { a.*(o.at) = a.*in_at + last; }});
                cases.push_back({std::string(o.name) + "=" + i.name + "+end", [o, in_at, in_bytes](Crypt& a) { a.*(o.at) = a.*in_at + in_bytes; }});
            };
            for (const In& i : ins) add(i);
            for (size_t y = 0; y < outs.size(); ++y)
                if (y != x) add(outs[y]);
        }
        // in place: the two sides are shifted against each other, so the same address is an overlap like any other
        cases.push_back({"d_out=d_in", [](Crypt& a) { a.d_out = a.d_in; }});
        // the output ends inside the input, and where the input begins
        cases.push_back({"d_out=d_in-bytes+16", [=](Crypt& a) { a.d_out = a.d_in - (decrypt ? msg : cph) + 16; }});
        cases.push_back({"d_out=d_in-bytes", [=](Crypt& a) { a.d_out = a.d_in - (decrypt ? msg : cph); }});
        run_cases(sym, good, cases, [decrypt](const Crypt& a) { return call(decrypt, a); });
    }
    {  // p252_encryption_tags takes no context: the message column stays empty
        uint64_t* out = new uint64_t[4 * (P252_CRYPT_RAGGED_MAX_LEN + 1)];
        const struct {
            const char* name;
            int variant;
            size_t max_len;
            bool null;
        } rows[] = {{"control", P252_CRYPT_STREAM, 42, false},  {"variant=DUPLEX", P252_CRYPT_DUPLEX, 42, false}, {"variant=2", 2, 42, false},
                    {"max_len=0", P252_CRYPT_STREAM, 0, false}, {"max_len=1", P252_CRYPT_STREAM, 1, false},
                    {"max_len=cap", P252_CRYPT_STREAM, P252_CRYPT_RAGGED_MAX_LEN, false},
                    {"max_len=cap+1", P252_CRYPT_STREAM, P252_CRYPT_RAGGED_MAX_LEN + 1, false},
                    {"max_len=SIZE_MAX", P252_CRYPT_STREAM, SIZE_MAX, false}, {"tags_out=NULL", P252_CRYPT_STREAM, 42, true}};
        for (const auto& r : rows) print_row("p252_encryption_tags", r.name, p252_encryption_tags(r.variant, r.max_len, r.null ? nullptr : out), "");
        delete[] out;
    }
    delete ctx;
    return 0;
}
