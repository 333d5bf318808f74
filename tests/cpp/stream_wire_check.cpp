// stream_wire_check.cpp — mpc_amd/csrc/stream_wire.h on the CPU (tests/test_stream_wire_host.py compiles and runs this under
// AddressSanitizer and UBSan).  argv[1] is a case file the Python side wrote; its lines are replayed in order:
//   fresh                                       a new WireStamps
//   gen N                                       the stamps' generation counter becomes N
//   walk NGATES NTMP NWIRES EXPECT USED HEX     walk_block over the bytes (a heap buffer of exactly their length) on the current
//                                               stamps; EXPECT = ok | rows | gate | arg is the exact status it must return,
//                                               USED the bytes an accepted block takes (0 otherwise)
//   step NGATES CW NIN NOUT NTMP NWIRES         a garbler step and the oracle's bytes for it, followed by
//     gates  (in0 in1 out op) x NGATES
//     in / out  the global ids
//     bytes  HEX
//     parse  (pos op flags short id0 id1 id2 rowpos nrows) x NGATES: tests/hostile_fuzz.py's reading of the bytes
// The exit status is 0 when every line holds; the first one that does not is reported on stderr.
#include <cstdio>
#include <fstream>
#include <map>
#include <memory>
#include <set>
#include <sstream>
#include <string>

#include "../../include/gcengine.h"
#include "stream_wire.h"

#define CHECK(cond)                                                                                        \
    do {                                                                                                   \
        if (!(cond)) {                                                                                     \
            std::fprintf(stderr, "%s:%d (case line %d): %s does not hold\n", __FILE__, __LINE__, g_line, #cond); \
            return 1;                                                                                      \
        }                                                                                                  \
    } while (0)

namespace {

int g_line = 0;

struct Bytes {  // a heap buffer of exactly n bytes (n == 0: a valid pointer to nothing)
    std::unique_ptr<uint8_t[]> p;
    size_t n = 0;
};
Bytes from_hex(const std::string &h) {
    Bytes b;
    b.n = h == "-" ? 0 : h.size() / 2;
    b.p.reset(new uint8_t[b.n]);
    auto nib = [](char c) { return (uint8_t)(c <= '9' ? c - '0' : c - 'a' + 10); };
    for (size_t i = 0; i < b.n; i++) b.p[i] = (uint8_t)(nib(h[2 * i]) << 4 | nib(h[2 * i + 1]));
    return b;
}

struct Sink {  // what the batch evaluator's sink keeps, and the fields as the single-session one numbers them
    std::vector<gcw::ParsedGate> gates;
    std::vector<uint32_t> row_off, fields;
    uint32_t global_field(size_t at, bool is_short) {
        fields.push_back((uint32_t)at | (is_short ? 0u : 0x80000000u));
        return (uint32_t)fields.size() - 1;
    }
    void gate(uint32_t g, uint32_t in0, uint32_t in1, uint32_t op, bool writes_tmp) {
        if (gates.size() <= g) gates.resize(g + 1);
        gates[g] = gcw::ParsedGate{in0, in1, op, writes_tmp};
    }
    void rows(size_t at, uint32_t n) {
        for (uint32_t r = 0; r < n; r++) row_off.push_back((uint32_t)(at + 16u * r));
    }
};

int walk(std::istringstream &ls, gcw::WireStamps &st) {
    uint32_t ngates, ntmp, nwires;
    std::string expect, hex;
    size_t want_used = 0;
    ls >> ngates >> ntmp >> nwires >> expect >> want_used >> hex;
    const Bytes b = from_hex(hex);
    gcw::BlockIo io;
    Sink sink;
    size_t used = ~(size_t)0;
    const int rc = gcw::walk_block(b.p.get(), b.n, ngates, ntmp, nwires, st, io, sink, &used);
    const int want = expect == "ok" ? GC_OK : expect == "rows" ? GC_E_ROWS : expect == "gate" ? GC_E_GATE : GC_E_ARG;
    CHECK(expect == "ok" || expect == "rows" || expect == "gate" || expect == "arg");
    CHECK(rc == want);
    if (rc == GC_OK) CHECK(used == want_used && used <= b.n && sink.gates.size() == ngates);
    return 0;
}

struct ParsedRef {
    uint32_t pos, op, flags, shortf, id[3], rowpos, nrows;
};

int step(std::istringstream &ls, std::ifstream &f) {
    uint32_t ngates, cw, nin, nout, ntmp, nwires;
    ls >> ngates >> cw >> nin >> nout >> ntmp >> nwires;
    std::vector<gc_gate> gates(ngates);
    std::vector<uint32_t> in(nin), out(nout);
    std::vector<ParsedRef> ref(ngates);
    std::string word, hex;
    f >> word;
    CHECK(word == "gates");
    for (auto &q : gates) {
        uint32_t op;
        f >> q.in0 >> q.in1 >> q.out >> op;
        q.op = (uint8_t)op;
    }
    f >> word;
    CHECK(word == "in");
    for (auto &v : in) f >> v;
    f >> word;
    CHECK(word == "out");
    for (auto &v : out) f >> v;
    f >> word >> hex;
    CHECK(word == "bytes");
    f >> word;
    CHECK(word == "parse");
    for (auto &r : ref) f >> r.pos >> r.op >> r.flags >> r.shortf >> r.id[0] >> r.id[1] >> r.id[2] >> r.rowpos >> r.nrows;
    CHECK(!f.fail());
    g_line += 4;  // (the rest of the parse line is read as an empty line)
    const Bytes want = from_hex(hex);

    // the writer: gate_form + put_gate_head reproduce the oracle's bytes outside the table rows, and their length
    std::vector<uint8_t> got(want.n, 0);
    size_t pos = 0;
    for (uint32_t g = 0; g < ngates; g++) {
        const gcw::GateForm q = gcw::gate_form(gates[g].op, gates[g].in0, gates[g].in1, gates[g].out, nin, cw - nout, in.data(), out.data());
        CHECK(q.rows == gcw::rows_of(gates[g].op) && q.wc == gcw::wires_of(gates[g].op));
        CHECK(q.size == 1 + (q.shortf ? 2u : 4u) * q.wc + 16u * q.rows && pos + q.size <= want.n);
        const uint8_t *row = gcw::put_gate_head(got.data() + pos, q);
        CHECK(row + 16 * q.rows == got.data() + pos + q.size);
        CHECK(pos == ref[g].pos && (size_t)(row - got.data()) == ref[g].rowpos && q.rows == ref[g].nrows);
        std::memcpy(got.data() + ref[g].rowpos, want.p.get() + ref[g].rowpos, 16 * q.rows);  // (the rows are the oracle's)
        pos += q.size;
    }
    CHECK(pos == want.n);
    CHECK(std::memcmp(got.data(), want.p.get(), want.n) == 0);

    // the reader, gate by gate: read_gate sees what the Python reading sees
    pos = 0;
    for (uint32_t g = 0; g < ngates; g++) {
        gcw::GateView v;
        CHECK(pos == ref[g].pos);
        CHECK(gcw::read_gate(want.p.get(), want.n, &pos, &v) == GC_OK);
        const uint32_t flags = (v.tmp0 ? 0x80u : 0) | (v.tmp1 ? 0x40u : 0) | (v.tmp_out ? 0x20u : 0);
        CHECK(v.op == ref[g].op && flags == ref[g].flags && v.shortf == (ref[g].shortf != 0));
        CHECK(v.nw == (ref[g].op == GC_INV ? 2u : 3u) && v.rows == ref[g].nrows);
        for (uint32_t i = 0; i < v.nw; i++) CHECK(v.w[i] == ref[g].id[i]);
        CHECK(v.id_off == ref[g].pos + 1 && v.row_off == ref[g].rowpos && pos == v.row_off + 16u * v.rows);
    }
    CHECK(pos == want.n);

    // the block walk: accepted whole, gates, row offsets and global fields as the Python reading has them
    gcw::WireStamps st;
    gcw::BlockIo io;
    Sink sink;
    size_t used = 0;
    CHECK(gcw::walk_block(want.p.get(), want.n, ngates, ntmp, nwires, st, io, sink, &used) == GC_OK);
    CHECK(used == want.n && sink.gates.size() == ngates);
    std::vector<uint32_t> rows_ref, fields_ref, writers_ref;
    std::map<uint32_t, uint32_t> last_writer;
    for (uint32_t g = 0; g < ngates; g++) {
        const ParsedRef &r = ref[g];
        CHECK(sink.gates[g].op == r.op && sink.gates[g].writes_tmp == ((r.flags & 0x20) != 0));
        for (uint32_t k = 0; k < r.nrows; k++) rows_ref.push_back(r.rowpos + 16 * k);
        const uint32_t nw = r.op == GC_INV ? 2 : 3, idsz = r.shortf ? 2 : 4;
        const uint32_t tmp[3] = {r.flags & 0x80, nw == 3 ? r.flags & 0x40 : r.flags & 0x20, r.flags & 0x20};
        for (uint32_t i = 0; i < nw; i++)
            if (!tmp[i]) fields_ref.push_back((r.pos + 1 + idsz * i) | (r.shortf ? 0u : 0x80000000u));
        if (!(r.flags & 0x20)) {
            writers_ref.push_back(g);
            last_writer[r.id[nw - 1]] = g;
        }
    }
    CHECK(sink.row_off == rows_ref && sink.fields == fields_ref);
    CHECK(io.writers.size() == writers_ref.size() && io.out_field.size() == io.writers.size());
    CHECK(io.in_field.size() == io.inputs.size());
    for (size_t k = 0; k < io.writers.size(); k++) {
        const uint32_t g = (uint32_t)(io.writers[k] >> 32), nw = ref[g].op == GC_INV ? 2 : 3;
        CHECK(g == writers_ref[k] && (uint32_t)io.writers[k] == ref[g].id[nw - 1]);
    }
    CHECK(std::set<uint32_t>(io.inputs.begin(), io.inputs.end()).size() == io.inputs.size());

    // the last writer of every global id stores it, and nobody else
    std::vector<uint8_t> live;
    gcw::live_outputs(st, io, &live);
    CHECK(live.size() == io.writers.size());
    for (size_t k = 0; k < live.size(); k++) CHECK((live[k] != 0) == (last_writer[(uint32_t)io.writers[k]] == (uint32_t)(io.writers[k] >> 32)));

    // the single-assignment list: every out distinct; every operand an input or the out of an earlier gate, and below its
    // gate's own out; inputs, then the tmp-writing gates, then the global-writing ones
    const uint32_t n_in = (uint32_t)io.inputs.size(), n_out = (uint32_t)io.writers.size();
    std::vector<uint32_t> id_of;
    std::vector<gc_gate> ssa;
    gcw::ssa_gate_list(sink.gates, n_in, n_out, [](const gcw::ParsedGate &p) { return p.writes_tmp; }, &id_of, &ssa);
    CHECK(ssa.size() == ngates && id_of.size() == ngates);
    std::set<uint32_t> defined;
    for (uint32_t g = 0; g < ngates; g++) {
        const gc_gate &q = ssa[g];
        CHECK(q.op == ref[g].op && q.out == id_of[g] && q.out >= n_in && q.out < n_in + ngates);
        CHECK((q.out >= n_in + ngates - n_out) == !sink.gates[g].writes_tmp);
        CHECK(q.in0 < n_in || defined.count(q.in0));
        CHECK(q.in0 < n_in || q.in0 < q.out);
        if (q.op != GC_INV) {
            CHECK(q.in1 < n_in || defined.count(q.in1));
            CHECK(q.in1 < n_in || q.in1 < q.out);
        } else {
            CHECK(q.in1 == 0);
        }
        CHECK(defined.insert(q.out).second);
    }
    return 0;
}

}  // namespace

int main(int argc, char **argv) {
    if (argc != 2) return 2;
    std::ifstream f(argv[1]);
    if (!f) return 2;
    gcw::WireStamps st;
    std::string line;
    int walks = 0, steps = 0;
    while (std::getline(f, line)) {
        g_line++;
        std::istringstream ls(line);
        std::string what;
        if (!(ls >> what)) continue;
        int rc = 0;
        if (what == "fresh") st = gcw::WireStamps();
        else if (what == "gen") ls >> st.gen;
        else if (what == "walk") rc = walk(ls, st), walks++;
        else if (what == "step") rc = step(ls, f), steps++;
        else rc = 2;
        if (rc) return rc;
    }
    std::printf("%d walks, %d steps\n", walks, steps);
    return 0;
}
