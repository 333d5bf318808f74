// mpc_host.hpp — C++ host-side mirror of the reference's Go API for the hot path, on top of the C ABI.
//
// The reference is Go; this image has no Go toolchain, so next to the cgo shim source (go/) the host side
// is mirrored here in C++ with the same names, argument meaning and error behaviour:
//
//   mpc::ot::Label / Wire                     ot/label.go:18-166
//   mpc::ot::IO, Pipe                         ot/io.go:15-47, ot/pipe.go:22-135
//   mpc::ot::OT (interface)                   ot/ot.go:16-28
//   mpc::ot::IKNPSender / IKNPReceiver        ot/iknp.go:80-226, 313-511   (semi-honest path)
//   mpc::ot::MITCCRH, COT                     ot/mitccrh.go:50-128, ot/cot.go:51-235
//   mpc::circuit::Operation / Gate / Circuit  circuit/circuit.go:22-34,120-131,260-266
//   Circuit::Garble / Circuit::Eval / Garbled circuit/garble.go:162-183,248-308, circuit/eval.go:17-115
//   mpc::circuit::ParseBristol                circuit/parser.go:265-494
//   mpc::circuit::Streaming                   circuit/stream_garble.go:41-192
//   mpc::sha2pc::GarblerBatch / EvaluatorBatch sha2pc/garbler.go:37-136, evaluator.go:27-113 for S sessions per call
//   mpc::rand::DeviceRand                     env.Config.Rand = cipher.StreamReader{cipher.NewCTR(...), zeros} for S sessions
//
// Go `error` returns become exceptions of type mpc::Error whose what() carries the reference's message.
// Go io.Reader becomes mpc::Reader.  Everything compute-heavy goes through libgcengine.so; there is no
// CPU fallback.
#pragma once

#include <cstdint>
#include <cstring>
#include <deque>
#include <memory>
#include <mutex>
#include <sstream>
#include <stdexcept>
#include <string>
#include <vector>

#include "gcengine.h"

namespace mpc {

struct Error : std::runtime_error {
    using std::runtime_error::runtime_error;
};

// io.Reader
struct Reader {
    virtual ~Reader() = default;
    virtual void Read(uint8_t *buf, size_t n) = 0;  // throws mpc::Error("unexpected EOF") when exhausted
};
struct BytesReader : Reader {
    std::vector<uint8_t> data;
    size_t pos = 0;
    explicit BytesReader(std::vector<uint8_t> d) : data(std::move(d)) {}
    void Read(uint8_t *buf, size_t n) override {
        if (pos + n > data.size()) throw Error("unexpected EOF");
        std::memcpy(buf, data.data() + pos, n);
        pos += n;
    }
};

inline void check(int st, const char *what) {
    if (st == GC_OK) return;
    std::string msg;
    switch (st) {
    case GC_E_KEYSIZE: msg = "crypto/aes: invalid key size"; break;
    case GC_E_GATE: msg = "invalid gate type"; break;
    case GC_E_ROWS: msg = "corrupted circuit"; break;
    default: msg = std::string(what) + ": " + gc_strerror(st) + " " + gc_last_error();
    }
    throw Error(msg);
}

// one device context per process unless the caller makes more (gc_ctx is one HIP device + stream)
class Context {
public:
    explicit Context(int device = 0) {
        int st = GC_OK;
        h_ = gc_ctx_create(device, &st);
        check(st, "gc_ctx_create");
    }
    ~Context() { gc_ctx_destroy(h_); }
    Context(const Context &) = delete;
    Context &operator=(const Context &) = delete;
    gc_ctx *handle() const { return h_; }
    static Context &Default() {
        static Context c(0);
        return c;
    }

private:
    gc_ctx *h_ = nullptr;
};

namespace ot {

// ot.Label (label.go:28-166).  Same memory layout as gc_label / Go's struct.
struct Label {
    uint64_t D0 = 0, D1 = 0;
    bool Equal(const Label &o) const { return D0 == o.D0 && D1 == o.D1; }
    bool S() const { return (D0 & 0x8000000000000000ull) != 0; }
    void SetS(bool set) {
        if (set) D0 |= 0x8000000000000000ull;
        else D0 &= 0x7fffffffffffffffull;
    }
    void Mul2() {
        D0 <<= 1;
        D0 |= D1 >> 63;
        D1 <<= 1;
    }
    void Mul4() {
        D0 <<= 2;
        D0 |= D1 >> 62;
        D1 <<= 2;
    }
    void Xor(const Label &o) {
        D0 ^= o.D0;
        D1 ^= o.D1;
    }
    unsigned Bit(int i) const {
        if (i < 0 || i > 127) throw Error("invalid bit index");
        return (unsigned)(((i > 63 ? D1 : D0) >> (i & 63)) & 1);
    }
    void GetData(uint8_t buf[16]) const {
        for (int i = 0; i < 8; i++) {
            buf[i] = (uint8_t)(D0 >> (56 - 8 * i));
            buf[8 + i] = (uint8_t)(D1 >> (56 - 8 * i));
        }
    }
    void SetData(const uint8_t buf[16]) {
        D0 = D1 = 0;
        for (int i = 0; i < 8; i++) {
            D0 = (D0 << 8) | buf[i];
            D1 = (D1 << 8) | buf[8 + i];
        }
    }
    std::string String() const {
        char b[40];
        std::snprintf(b, sizeof b, "%016llx%016llx", (unsigned long long)D0, (unsigned long long)D1);
        return b;
    }
};
static_assert(sizeof(Label) == sizeof(gc_label), "Label layout");

inline Label NewLabel(Reader &rand) {  // label.go:46-55
    uint8_t buf[16];
    rand.Read(buf, 16);
    Label l;
    l.SetData(buf);
    return l;
}

struct Wire {
    Label L0, L1;
};
static_assert(sizeof(Wire) == sizeof(gc_wire), "Wire layout");

// ot.IO (io.go:15-47) — the subset the hot path uses
struct IO {
    virtual ~IO() = default;
    virtual void SendData(const std::vector<uint8_t> &d) = 0;
    virtual std::vector<uint8_t> ReceiveData() = 0;
    virtual void Flush() {}
    void SendLabel(const Label &l) {
        std::vector<uint8_t> b(16);
        l.GetData(b.data());
        SendData(b);
    }
    Label ReceiveLabel() {
        auto b = ReceiveData();
        if (b.size() != 16) throw Error("invalid label length");
        Label l;
        l.SetData(b.data());
        return l;
    }
};

// ot.Pipe (pipe.go): in-memory IO for single-threaded, strictly alternating protocols (tests)
class Pipe : public IO {
public:
    static std::pair<std::shared_ptr<Pipe>, std::shared_ptr<Pipe>> New() {
        auto a = std::make_shared<Pipe>(), b = std::make_shared<Pipe>();
        a->peer_ = b.get();
        b->peer_ = a.get();
        return {a, b};
    }
    void SendData(const std::vector<uint8_t> &d) override {
        if (d.size() > 64 * 1024) throw Error("pipe: message too long");  // pipe.go:62-71
        peer_->q_.push_back(d);
    }
    std::vector<uint8_t> ReceiveData() override {
        if (q_.empty()) throw Error("EOF");
        auto d = std::move(q_.front());
        q_.pop_front();
        return d;
    }

private:
    Pipe *peer_ = nullptr;
    std::deque<std::vector<uint8_t>> q_;
};

// ot.OT (ot.go:16-28)
struct OT {
    virtual ~OT() = default;
    virtual void InitSender(IO &io) = 0;
    virtual void InitReceiver(IO &io) = 0;
    virtual void Send(const std::vector<Wire> &wires) = 0;
    virtual void Receive(const std::vector<bool> &flags, std::vector<Label> &result) = 0;
};

constexpr int K = 128;                  // iknp.go:64-67
constexpr size_t chunkSize = 8 * 1024;  // iknp.go:70

// MITCCRH over a run of OTs (mitccrh.go:93-128 as driven by cot.go:160-171)
inline void MITCCRHHash(Context &ctx, const Label &seed, uint64_t gid0, std::vector<Label> &blks, uint32_t h) {
    if (blks.empty()) return;
    check(gc_mitccrh_hash(ctx.handle(), (const gc_label *)&seed, gid0, (gc_label *)blks.data(), blks.size() / h, h),
          "gc_mitccrh_hash");
}

class IKNPSender {
public:
    Label Delta;
    // NewIKNPSender (iknp.go:89-127): k0[i] = the base-OT result for choice Delta.Bit(i)
    IKNPSender(Context &ctx, OT &base, IO &io, Reader &r, const Label *d = nullptr) : ctx_(ctx), io_(io) {
        Delta = d ? *d : NewLabel(r);
        std::vector<bool> flags(K);
        for (int i = 0; i < K; i++) flags[i] = Delta.Bit(i) == 1;
        std::vector<Label> k0(K);
        base.Receive(flags, k0);
        int st = GC_OK;
        h_ = gc_iknp_sender_create(ctx.handle(), (const gc_label *)&Delta, (const gc_label *)k0.data(), &st);
        check(st, "gc_iknp_sender_create");
    }
    ~IKNPSender() { gc_iknp_free(h_); }
    // Send (iknp.go:129, semi-honest): returns b0; b1 = b0 ^ Delta
    std::vector<Label> Send(int n) {
        std::vector<Label> result((size_t)n);
        const size_t want = gc_iknp_u_bytes((size_t)n);
        std::vector<uint8_t> u;
        while (u.size() < want) {  // send(): one ReceiveData per chunk (iknp.go:202-209)
            auto chunk = io_.ReceiveData();
            if (chunk.size() % K != 0) throw Error("invalid chunk size: " + std::to_string(chunk.size()));
            u.insert(u.end(), chunk.begin(), chunk.end());
        }
        if (n) check(gc_iknp_send(h_, u.data(), u.size(), (size_t)n, (gc_label *)result.data()), "gc_iknp_send");
        return result;
    }

private:
    Context &ctx_;
    IO &io_;
    gc_iknp *h_ = nullptr;
};

class IKNPReceiver {
public:
    // NewIKNPReceiver (iknp.go:321-361)
    IKNPReceiver(Context &ctx, OT &base, IO &io, Reader &rand) : ctx_(ctx), io_(io) {
        std::vector<Wire> wires(K);
        for (int i = 0; i < K; i++) {
            wires[i].L0 = NewLabel(rand);
            wires[i].L1 = NewLabel(rand);
        }
        base.Send(wires);
        int st = GC_OK;
        h_ = gc_iknp_receiver_create(ctx.handle(), (const gc_wire *)wires.data(), &st);
        check(st, "gc_iknp_receiver_create");
    }
    ~IKNPReceiver() { gc_iknp_free(h_); }
    // Receive (iknp.go:364, semi-honest): result[i] = b0[i] ^ b[i]*Delta
    void Receive(const std::vector<bool> &b, std::vector<Label> &result) {
        if (b.size() != result.size()) throw Error("len(b) != len(result)");
        const size_t n = b.size();
        if (n) {
            std::vector<uint8_t> choice(n), u(gc_iknp_u_bytes(n));
            for (size_t i = 0; i < n; i++) choice[i] = b[i] ? 1 : 0;
            check(gc_iknp_receive(h_, choice.data(), n, u.data(), (gc_label *)result.data()), "gc_iknp_receive");
            for (size_t ofs = 0; ofs < u.size(); ofs += chunkSize)  // SendData per chunk (iknp.go:499)
                io_.SendData(std::vector<uint8_t>(u.begin() + (long)ofs,
                                                  u.begin() + (long)std::min(u.size(), ofs + chunkSize)));
        }
        io_.Flush();
    }

private:
    Context &ctx_;
    IO &io_;
    gc_iknp *h_ = nullptr;
};

// ot.COT (cot.go:51-235), semi-honest
class COT : public OT {
public:
    COT(Context &ctx, OT &base, Reader &r) : ctx_(ctx), base_(base), r_(r) {}
    void InitSender(IO &io) override {
        if (iknpR_) throw Error("already initialized as receiver");
        if (iknpS_) throw Error("already initialized");
        base_.InitSender(io);
        iknpS_ = std::make_unique<IKNPSender>(ctx_, base_, io, r_);
        io_ = &io;
    }
    void InitReceiver(IO &io) override {
        if (iknpS_) throw Error("already initialized as sender");
        if (iknpR_) throw Error("already initialized");
        base_.InitReceiver(io);
        iknpR_ = std::make_unique<IKNPReceiver>(ctx_, base_, io, r_);
        io_ = &io;
    }
    void Send(const std::vector<Wire> &wires) override {  // cot.go:136-185
        if (!iknpS_) throw Error("not initialized as sender");
        auto data = iknpS_->Send((int)wires.size());
        Label seed = NewLabel(r_);
        io_->SendLabel(seed);
        io_->Flush();
        std::vector<Label> out(2 * wires.size());
        if (!wires.empty())
            check(gc_cot_send_pads(ctx_.handle(), (const gc_label *)&seed, (const gc_label *)&iknpS_->Delta,
                                   (const gc_label *)data.data(), (const gc_wire *)wires.data(), wires.size(),
                                   (gc_label *)out.data()),
                  "gc_cot_send_pads");
        for (const Label &l : out) io_->SendLabel(l);
        io_->Flush();
    }
    void Receive(const std::vector<bool> &flags, std::vector<Label> &result) override {  // cot.go:187-235
        if (!iknpR_) throw Error("not initialized as receiver");
        iknpR_->Receive(flags, result);
        pending_flags_ = flags;
        pending_ = &result;
    }
    // second half of COT.Receive once the sender's messages are in the pipe (single-threaded tests run
    // the two parties in lock-step; a threaded driver calls Receive() then FinishReceive() back to back)
    void FinishReceive() {
        std::vector<Label> &result = *pending_;
        Label seed = io_->ReceiveLabel();
        std::vector<Label> sent(2 * result.size());
        for (auto &l : sent) l = io_->ReceiveLabel();
        std::vector<uint8_t> f(result.size());
        for (size_t i = 0; i < f.size(); i++) f[i] = pending_flags_[i] ? 1 : 0;
        if (!result.empty())
            check(gc_cot_receive_unpad(ctx_.handle(), (const gc_label *)&seed, f.data(), (const gc_label *)sent.data(),
                                       (gc_label *)result.data(), result.size()),
                  "gc_cot_receive_unpad");
    }
    IKNPSender *sender() { return iknpS_.get(); }

private:
    Context &ctx_;
    OT &base_;
    Reader &r_;
    IO *io_ = nullptr;
    std::unique_ptr<IKNPSender> iknpS_;
    std::unique_ptr<IKNPReceiver> iknpR_;
    std::vector<bool> pending_flags_;
    std::vector<Label> *pending_ = nullptr;
};

}  // namespace ot

namespace circuit {

// circuit.Operation (circuit.go:25-34)
enum Operation : uint8_t { XOR = 0, XNOR = 1, AND = 2, OR = 3, INV = 4 };
inline const char *OperationString(Operation op) {
    static const char *n[] = {"XOR", "XNOR", "AND", "OR", "INV"};
    return op <= INV ? n[op] : "{Operation}";
}

using Wire = uint32_t;

// circuit.Gate (circuit.go:260-266), 20 bytes like Go's (circuit_test.go:14-19)
struct Gate {
    Wire Input0, Input1, Output;
    Operation Op;
    uint32_t Level;
};
static_assert(sizeof(Gate) == 20 && sizeof(Gate) == sizeof(gc_gate), "Gate layout");

class Circuit;

// circuit.Garbled (garble.go:162-183)
struct Garbled {
    ot::Label R;
    std::vector<ot::Wire> Wires;
    std::vector<std::pair<const ot::Label *, size_t>> Gates;  // (rows, count) per gate; (nullptr,0) for free gates
    std::vector<ot::Label> slab;                             // backing store of Gates
    void Release() {}                                        // scratch is owned by value here
};

class Circuit {
public:
    int NumGates = 0, NumWires = 0;
    std::vector<int> Inputs, Outputs;  // IO sizes in bits (IO.Size() = sum)
    std::vector<Gate> Gates;

    int InputsSize() const { return sum(Inputs); }
    int OutputsSize() const { return sum(Outputs); }

    // Garble (garble.go:248-308)
    Garbled Garble(Reader &rand, const std::vector<uint8_t> &key, Context &ctx = Context::Default()) {
        const int nin = InputsSize();
        std::vector<uint8_t> rnd(16 * ((size_t)nin + 1));
        rand.Read(rnd.data(), 16);                               // R             (:253)
        if (key.size() != 16 && key.size() != 24 && key.size() != 32)
            throw Error("crypto/aes: invalid key size " + std::to_string(key.size()));  // (:260)
        rand.Read(rnd.data() + 16, 16 * (size_t)nin);             // input labels  (:271-278)
        gc_circ *c = device(ctx);
        gc_plan_info info;
        gc_plan_get_info(gc_circ_plan(c), &info);
        Garbled g;
        g.Wires.resize((size_t)NumWires);
        g.slab.resize(info.slab_rows);
        check(gc_garble(c, key.data(), key.size(), rnd.data(), rnd.size(), 1, (gc_label *)&g.R,
                        (gc_wire *)g.Wires.data(), nullptr, (gc_label *)g.slab.data()),
              "gc_garble");
        g.Gates.resize(Gates.size());
        size_t off = 0;
        for (size_t i = 0; i < Gates.size(); i++) {
            size_t n = Gates[i].Op == AND ? 2 : Gates[i].Op == OR ? 3 : Gates[i].Op == INV ? 1 : 0;
            g.Gates[i] = {n ? g.slab.data() + off : nullptr, n};
            off += n;
        }
        return g;
    }

    // Eval (eval.go:17-115): wires (len NumWires, inputs pre-filled) is written in place
    void Eval(const std::vector<uint8_t> &key, std::vector<ot::Label> &wires,
              const std::vector<std::pair<const ot::Label *, size_t>> &garbled, Context &ctx = Context::Default()) {
        if (key.size() != 16 && key.size() != 24 && key.size() != 32)
            throw Error("crypto/aes: invalid key size " + std::to_string(key.size()));
        std::vector<ot::Label> slab;
        for (size_t i = 0; i < Gates.size(); i++) {
            const auto &row = garbled[i];
            switch (Gates[i].Op) {
            case AND:
                if (row.second != 2) throw Error("corrupted ciruit: AND row length: " + std::to_string(row.second));
                break;
            case OR:
                if (row.second < 3) throw Error("corrupted circuit: index " + std::to_string(row.second) + " >= row " + std::to_string(row.second));
                break;
            case INV:
                if (row.second < 1) throw Error("corrupted circuit: index 0 >= row 0");
                break;
            default: continue;
            }
            slab.insert(slab.end(), row.first, row.first + row.second);
        }
        gc_circ *c = device(ctx);
        check(gc_eval(c, key.data(), key.size(), 1, (gc_label *)wires.data(), nullptr, (const gc_label *)slab.data(),
                      slab.size(), nullptr),
              "gc_eval");
    }

    ~Circuit() {
        if (circ_) gc_circ_free(circ_);
    }
    Circuit() = default;
    Circuit(Circuit &&o) noexcept { *this = std::move(o); }
    Circuit &operator=(Circuit &&o) noexcept {
        NumGates = o.NumGates;
        NumWires = o.NumWires;
        Inputs = std::move(o.Inputs);
        Outputs = std::move(o.Outputs);
        Gates = std::move(o.Gates);
        circ_ = o.circ_;
        o.circ_ = nullptr;
        return *this;
    }

    gc_circ *device(Context &ctx) {
        std::lock_guard<std::mutex> lk(mu_);
        if (!circ_) {
            int st = GC_OK;
            circ_ = gc_circ_load(ctx.handle(), (const gc_gate *)Gates.data(), (uint32_t)Gates.size(), (uint32_t)NumWires,
                                 (uint32_t)InputsSize(), (uint32_t)OutputsSize(), &st);
            if (st == GC_E_GATE) throw Error("invalid gate type");
            check(st, "gc_circ_load");
        }
        return circ_;
    }

private:
    static int sum(const std::vector<int> &v) {
        int s = 0;
        for (int x : v) s += x;
        return s;
    }
    gc_circ *circ_ = nullptr;
    std::mutex mu_;
};

// Many Garbler / Evaluator sessions gathered into one device-resident batch (gc_batch_*): every session drew its own key
// (garbler.go:47-53) and sent it to its peer (:64), so instance i is garbled and evaluated under key i.  d_keys = u8
// [batch][keylen] and d_rnd are device buffers (gc_dev_alloc); the calls enqueue on the ctx stream and do not wait.
// BatchKeysSupported: gc_batch_keyed_supported (schedule 1; wires in LDS and the key table fits, or wires in HBM).
// BatchKeysPath: gc_batch_keyed_path (0 none, 1 the flattened kernels with the wires in LDS, 2 the level-walking kernels with
// the wires in HBM); SetBatchKeysPath(b, 2) sends any schedule-1 batch to path 2, 0 restores the rule.
inline bool BatchKeysSupported(const gc_batch *b) { return gc_batch_keyed_supported(b) != 0; }
inline int BatchKeysPath(const gc_batch *b) { return gc_batch_keyed_path(b); }
inline void SetBatchKeysPath(gc_batch *b, int path) { check(gc_batch_set_keyed_path(b, path), "gc_batch_set_keyed_path"); }
// BatchKeysHbmForm: gc_batch_keyed_hbm_form (0 not on path 2, 1 the plain form of the HBM-wire kernels, 2 the split form with
// hash waves and free waves on wide levels); SetBatchKeysHbmForm: 0 the rule, 1 always plain, 2 always split
inline int BatchKeysHbmForm(const gc_batch *b) { return gc_batch_keyed_hbm_form(b); }
inline void SetBatchKeysHbmForm(gc_batch *b, int form) { check(gc_batch_set_keyed_hbm_form(b, form), "gc_batch_set_keyed_hbm_form"); }
inline void GarbleBatchKeys(gc_batch *b, const void *d_keys, size_t keylen, const void *d_rnd) {
    if (keylen != 16 && keylen != 24 && keylen != 32) throw Error("crypto/aes: invalid key size " + std::to_string(keylen));
    check(gc_batch_garble_keyed(b, d_keys, keylen, d_rnd), "gc_batch_garble_keyed");
}
inline void EvalBatchKeys(gc_batch *evaluator, const void *d_keys, size_t keylen, const gc_batch *tables) {
    if (keylen != 16 && keylen != 24 && keylen != 32) throw Error("crypto/aes: invalid key size " + std::to_string(keylen));
    check(gc_batch_eval_keyed(evaluator, d_keys, keylen, tables), "gc_batch_eval_keyed");
}

// S sessions of ONE streamed program per call (gc_stream_batch_*, gc_stream_eval_batch_*): a step is one keyed batch pass over S
// instances between a device-resident wire store per handle; session s's bytes are those of Streaming.Garble
// (stream_garble.go:161-192) with its own key and random stream.  d_* are device buffers (gc_dev_alloc).
class StreamingBatch {
public:
    StreamingBatch(gc_ctx *ctx, uint32_t sessions, const void *d_keys, size_t keylen, const void *d_rnd,
                   const std::vector<uint32_t> &inputs)
        : sessions_(sessions) {
        int st = GC_OK;
        h_ = gc_stream_batch_create(ctx, sessions, d_keys, keylen, d_rnd, inputs.data(), (uint32_t)inputs.size(), &st);
        if (!h_) check(st, "gc_stream_batch_create");
    }
    ~StreamingBatch() { gc_stream_batch_free(h_); }
    StreamingBatch(const StreamingBatch &) = delete;
    StreamingBatch &operator=(const StreamingBatch &) = delete;
    static size_t StepBytes(const std::vector<gc_gate> &gates, uint32_t nwires, const std::vector<uint32_t> &in,
                            const std::vector<uint32_t> &out) {
        return gc_stream_batch_step_bytes(gates.data(), (uint32_t)gates.size(), nwires, in.data(), (uint32_t)in.size(), out.data(),
                                          (uint32_t)out.size());
    }
    // queues the step; session s's bytes land at d_out + s * stride; returns the step's byte count
    size_t Garble(const std::vector<gc_gate> &gates, uint32_t nwires, const std::vector<uint32_t> &in,
                  const std::vector<uint32_t> &out, void *d_out, size_t stride) {
        size_t n = 0;
        check(gc_stream_batch_garble(h_, gates.data(), (uint32_t)gates.size(), nwires, in.data(), (uint32_t)in.size(), out.data(),
                                     (uint32_t)out.size(), d_out, stride, &n),
              "gc_stream_batch_garble");
        return n;
    }
    std::vector<gc_wire> GetInput(uint32_t w) {
        std::vector<gc_wire> out(sessions_);
        check(gc_stream_batch_get_wire(h_, w, out.data()), "gc_stream_batch_get_wire");
        return out;
    }
    void GatherWires(const std::vector<uint32_t> &ids, void *d_wires_out) {
        check(gc_stream_batch_gather_wires(h_, ids.data(), (uint32_t)ids.size(), d_wires_out), "gc_stream_batch_gather_wires");
    }
    // the circuit cache: what it holds now, and how often it loaded and evicted
    struct CacheStats {
        uint64_t entries = 0, bytes = 0, loads = 0, evictions = 0;
    };
    CacheStats GetCacheStats() const {
        CacheStats c;
        check(gc_stream_batch_cache_stats(h_, &c.entries, &c.bytes, &c.loads, &c.evictions), "gc_stream_batch_cache_stats");
        return c;
    }
    // the garbler's own input labels (streamer.go:79-102): d_labels_out gc_label [sessions][ids] = L0, ^ R where d_bits (u8
    // [sessions][ids]) is not zero; asynchronous
    void SelectLabelsDev(const std::vector<uint32_t> &ids, const void *d_bits, void *d_labels_out) {
        check(gc_stream_batch_select_labels_dev(h_, ids.data(), (uint32_t)ids.size(), d_bits, d_labels_out),
              "gc_stream_batch_select_labels_dev");
    }
    // ... from host bits [sessions][ids], synchronous
    std::vector<gc_label> SelectLabels(const std::vector<uint32_t> &ids, const std::vector<uint8_t> &bits) {
        if (bits.size() != (size_t)sessions_ * ids.size()) throw Error("SelectLabels: bits must be [sessions][ids]");
        std::vector<gc_label> out(bits.size());
        check(gc_stream_batch_select_labels(h_, ids.data(), (uint32_t)ids.size(), bits.data(), out.data()),
              "gc_stream_batch_select_labels");
        return out;
    }
    // the result (streamer.go:563-579): d_bits_out u8 [sessions][ids] = 0 / 1 / 0xff ("unknown label"), d_bad u32 [sessions] =
    // the 0xff entries of a session; asynchronous
    void DecodeDev(const std::vector<uint32_t> &ids, const void *d_labels, void *d_bits_out, void *d_bad) {
        check(gc_stream_batch_decode_dev(h_, ids.data(), (uint32_t)ids.size(), d_labels, d_bits_out, d_bad),
              "gc_stream_batch_decode_dev");
    }
    // ... of host labels [sessions][ids], synchronous; bad: [sessions]
    std::vector<uint8_t> Decode(const std::vector<uint32_t> &ids, const std::vector<gc_label> &labels, std::vector<uint32_t> *bad) {
        if (labels.size() != (size_t)sessions_ * ids.size() || !bad) throw Error("Decode: labels must be [sessions][ids]");
        std::vector<uint8_t> bits(labels.size());
        bad->assign(sessions_, 0);
        check(gc_stream_batch_decode(h_, ids.data(), (uint32_t)ids.size(), labels.data(), bits.data(), bad->data()),
              "gc_stream_batch_decode");
        return bits;
    }
    // circuits loaded from now on that the key table alone keeps out of the keyed scope run on the HBM-wire kernels
    void SetFallback(bool on) { check(gc_stream_batch_set_fallback(h_, on ? 1 : 0), "gc_stream_batch_set_fallback"); }
    gc_stream_batch *handle() const { return h_; }
    uint32_t sessions() const { return sessions_; }

private:
    gc_stream_batch *h_ = nullptr;
    uint32_t sessions_;
};

// The steps of a StreamingBatch in windows of pinned host memory (gc_stream_batch_out_*): destroy it before its StreamingBatch.
// One thread may call Garble / Flush while one other calls Next / Release.
class StreamingBatchOut {
public:
    // split: a step is cut over the windows (gc_stream_batch_out_create_split): every window but a flushed one leaves exactly
    // full, none grows, and a step larger than nwindows - 1 windows is refused
    StreamingBatchOut(StreamingBatch &sb, size_t window_bytes, uint32_t nwindows, bool split = false) {
        int st = GC_OK;
        h_ = split ? gc_stream_batch_out_create_split(sb.handle(), window_bytes, nwindows, &st)
                   : gc_stream_batch_out_create(sb.handle(), window_bytes, nwindows, &st);
        if (!h_) check(st, split ? "gc_stream_batch_out_create_split" : "gc_stream_batch_out_create");
    }
    ~StreamingBatchOut() { gc_stream_batch_out_free(h_); }
    StreamingBatchOut(const StreamingBatchOut &) = delete;
    StreamingBatchOut &operator=(const StreamingBatchOut &) = delete;
    // false: no window is free (GC_E_BUSY) — nothing has happened; release one and call again.  *written: bytes per session,
    // the prefix (the OpCircuit header, streamer.go:679-693) included
    bool Garble(const std::vector<uint8_t> &prefix, const std::vector<gc_gate> &gates, uint32_t nwires,
                const std::vector<uint32_t> &in, const std::vector<uint32_t> &out, size_t *written) {
        size_t n = 0;
        const int st = gc_stream_batch_out_garble(h_, prefix.data(), prefix.size(), gates.data(), (uint32_t)gates.size(), nwires,
                                                  in.data(), (uint32_t)in.size(), out.data(), (uint32_t)out.size(), &n);
        if (written) *written = n;
        if (st == GC_E_BUSY) return false;
        check(st, "gc_stream_batch_out_garble");
        return true;
    }
    void Flush() { check(gc_stream_batch_out_flush(h_), "gc_stream_batch_out_flush"); }
    struct Window {
        const uint8_t *base = nullptr;  // session s's bytes: base + s * stride
        size_t stride = 0, len = 0;     // len == 0: nothing is sealed
    };
    Window Next() {
        Window w;
        check(gc_stream_batch_out_next(h_, &w.base, &w.stride, &w.len), "gc_stream_batch_out_next");
        return w;
    }
    void Release() { check(gc_stream_batch_out_release(h_), "gc_stream_batch_out_release"); }
    struct Stats {
        uint64_t sealed = 0, bytes_per_session = 0, grown = 0, busy = 0;
    };
    Stats GetStats() const {
        Stats s;
        check(gc_stream_batch_out_stats(h_, &s.sealed, &s.bytes_per_session, &s.grown, &s.busy), "gc_stream_batch_out_stats");
        return s;
    }
    struct SplitStats {
        uint64_t split_steps = 0, segments = 0;  // steps that touched more than one window, serialiser launches
    };
    SplitStats GetSplitStats() const {
        SplitStats s;
        check(gc_stream_batch_out_split_stats(h_, &s.split_steps, &s.segments), "gc_stream_batch_out_split_stats");
        return s;
    }

private:
    gc_stream_batch_out *h_ = nullptr;
};

class StreamEvalBatch {
public:
    StreamEvalBatch(gc_ctx *ctx, uint32_t sessions, const void *d_keys, size_t keylen) : sessions_(sessions) {
        int st = GC_OK;
        h_ = gc_stream_eval_batch_create(ctx, sessions, d_keys, keylen, &st);
        if (!h_) check(st, "gc_stream_eval_batch_create");
    }
    ~StreamEvalBatch() { gc_stream_eval_batch_free(h_); }
    StreamEvalBatch(const StreamEvalBatch &) = delete;
    StreamEvalBatch &operator=(const StreamEvalBatch &) = delete;
    void SetWires(const std::vector<uint32_t> &ids, const void *d_labels) {
        check(gc_stream_eval_batch_set_wires(h_, ids.data(), (uint32_t)ids.size(), d_labels), "gc_stream_eval_batch_set_wires");
    }
    std::vector<gc_label> Get(uint32_t w) {
        std::vector<gc_label> out(sessions_);
        check(gc_stream_eval_batch_get_wire(h_, w, out.data()), "gc_stream_eval_batch_get_wire");
        return out;
    }
    // one OpCircuit block of every session; d_bad: u32 [sessions], the structure bytes in which a block differs from ref
    size_t EvalBlock(uint32_t ngates, uint32_t ntmp, uint32_t nwires, const std::vector<uint8_t> &ref, const void *d_blocks,
                     size_t stride, void *d_bad) {
        size_t used = 0;
        check(gc_stream_eval_batch_circuit(h_, ngates, ntmp, nwires, ref.data(), ref.size(), d_blocks, stride, d_bad, &used),
              "gc_stream_eval_batch_circuit");
        return used;
    }
    // EvalBlock with every session's block in HOST memory, `stride` apart (a window of StreamingBatchOut: base + offset);
    // session ref_session's is the reference block.  Pinned memory stays untouched until UploadsWait / Bad returns.
    size_t EvalBlockHost(uint32_t ngates, uint32_t ntmp, uint32_t nwires, const uint8_t *blocks, size_t stride, size_t len,
                         uint32_t ref_session = 0) {
        size_t used = 0;
        check(gc_stream_eval_batch_circuit_host(h_, ngates, ntmp, nwires, blocks, stride, len, ref_session, &used),
              "gc_stream_eval_batch_circuit_host");
        return used;
    }
    void UploadsWait() { check(gc_stream_eval_batch_uploads_wait(h_), "gc_stream_eval_batch_uploads_wait"); }
    // blocks whose circuit is loaded from now on and kept out of the keyed scope by the key table alone run on the HBM-wire kernels
    void SetFallback(bool on) { check(gc_stream_eval_batch_set_fallback(h_, on ? 1 : 0), "gc_stream_eval_batch_set_fallback"); }
    // per session the structure bytes that differed in any EvalBlockHost since construction (waits)
    std::vector<uint32_t> Bad() {
        std::vector<uint32_t> bad(sessions_);
        check(gc_stream_eval_batch_bad(h_, bad.data()), "gc_stream_eval_batch_bad");
        return bad;
    }
    StreamingBatch::CacheStats GetCacheStats() const {
        StreamingBatch::CacheStats c;
        check(gc_stream_eval_batch_cache_stats(h_, &c.entries, &c.bytes, &c.loads, &c.evictions), "gc_stream_eval_batch_cache_stats");
        return c;
    }
    // OpReturn (stream_evaluator.go:434-461): gc_label [sessions][ids.size()] in device memory, what StreamingBatch's decode
    // reads; asynchronous
    void ReturnLabelsDev(const std::vector<uint32_t> &ids, void *d_labels_out) {
        check(gc_stream_eval_batch_return_labels_dev(h_, ids.data(), (uint32_t)ids.size(), d_labels_out),
              "gc_stream_eval_batch_return_labels_dev");
    }
    // ... the same into host memory: [s * ids.size() + j] = the active label of wire ids[j] in session s (waits)
    std::vector<gc_label> ReturnLabels(const std::vector<uint32_t> &ids) {
        std::vector<gc_label> out((size_t)sessions_ * ids.size());
        check(gc_stream_eval_batch_return_labels(h_, ids.data(), (uint32_t)ids.size(), out.data()), "gc_stream_eval_batch_return_labels");
        return out;
    }
    gc_stream_eval_batch *handle() { return h_; }
    uint32_t sessions() const { return sessions_; }

private:
    gc_stream_eval_batch *h_ = nullptr;
    uint32_t sessions_;
};

// The intake of a StreamEvalBatch (gc_stream_eval_batch_in_*): chunks of the S byte streams that respect no step boundary in,
// evaluated steps out.  Destroy it before its StreamEvalBatch; one thread feeds it at a time.
class StreamEvalBatchIn {
public:
    StreamEvalBatchIn(StreamEvalBatch &e, uint32_t ref_session, size_t max_message_bytes) {
        int st = GC_OK;
        h_ = gc_stream_eval_batch_in_create(e.handle(), ref_session, max_message_bytes, &st);
        if (!h_) check(st, "gc_stream_eval_batch_in_create");
    }
    ~StreamEvalBatchIn() { gc_stream_eval_batch_in_free(h_); }
    StreamEvalBatchIn(const StreamEvalBatchIn &) = delete;
    StreamEvalBatchIn &operator=(const StreamEvalBatchIn &) = delete;
    struct Fed {
        size_t taken = 0;      // bytes of the chunk that were taken
        uint32_t next_op = 1;  // 1 (OpCircuit): all of them; else the op word the feed stopped in front of
        int status = GC_OK;    // GC_E_GATE / GC_E_ROWS / GC_E_ARG: the message at `taken` was refused by the parser
    };
    // session s's next len bytes at chunk + s * stride.  A refused message is reported in Fed::status (the handle stays
    // usable); any other failure throws.
    Fed Feed(const uint8_t *chunk, size_t stride, size_t len) {
        Fed f;
        f.status = gc_stream_eval_batch_in_feed(h_, chunk, stride, len, &f.taken, &f.next_op);
        if (f.status != GC_E_GATE && f.status != GC_E_ROWS && f.status != GC_E_ARG) check(f.status, "gc_stream_eval_batch_in_feed");
        return f;
    }
    struct Stats {
        uint64_t steps = 0, bytes_per_session = 0, uploads = 0, carried_bytes = 0;
    };
    Stats GetStats() const {
        Stats s;
        check(gc_stream_eval_batch_in_stats(h_, &s.steps, &s.bytes_per_session, &s.uploads, &s.carried_bytes),
              "gc_stream_eval_batch_in_stats");
        return s;
    }

private:
    gc_stream_eval_batch_in *h_ = nullptr;
};

// ParseBristol (parser.go:265-494), same validation messages
inline Circuit ParseBristol(std::istream &in) {
    auto fail = [](const std::string &m) -> void { throw Error(m); };
    std::string line;
    auto next = [&](std::vector<std::string> &parts) {
        while (std::getline(in, line)) {
            std::istringstream ss(line);
            parts.clear();
            std::string t;
            while (ss >> t) parts.push_back(t);
            if (!parts.empty()) return true;
        }
        return false;
    };
    std::vector<std::string> p;
    Circuit c;
    if (!next(p) || p.size() != 2) fail("invalid 1st line: '" + line + "'");
    c.NumGates = std::stoi(p[0]);
    c.NumWires = std::stoi(p[1]);
    std::vector<bool> seen((size_t)c.NumWires, false);
    if (!next(p)) fail("EOF");
    if ((size_t)std::stoi(p[0]) + 1 != p.size()) fail("invalid inputs line: niv=" + p[0] + ", len=" + std::to_string(p.size()));
    long iw = 0;
    for (size_t i = 1; i < p.size(); i++) {
        c.Inputs.push_back(std::stoi(p[i]));
        iw += c.Inputs.back();
    }
    if (iw == 0) fail("no inputs defined");
    for (long i = 0; i < iw; i++) seen.at((size_t)i) = true;
    if (!next(p) || (size_t)std::stoi(p[0]) + 1 != p.size()) fail("invalid outputs line");
    for (size_t i = 1; i < p.size(); i++) c.Outputs.push_back(std::stoi(p[i]));
    int gate = 0;
    for (; next(p); gate++) {
        if (gate >= c.NumGates) fail("too many gates");
        if (p.size() < 3) fail("invalid gate: " + line);
        int n1 = std::stoi(p[0]), n2 = std::stoi(p[1]);
        if ((size_t)(2 + n1 + n2 + 1) != p.size()) fail("invalid gate: " + line);
        std::vector<Wire> ins, outs;
        for (int i = 0; i < n1; i++) {
            unsigned long v = std::stoul(p[2 + i]);
            if (v >= seen.size()) fail("invalid wire " + std::to_string(v) + " [0..." + std::to_string(seen.size()) + "[");
            if (!seen[v]) fail("input " + std::to_string(v) + " of gate " + std::to_string(gate) + " not set");
            ins.push_back((Wire)v);
        }
        for (int i = 0; i < n2; i++) {
            unsigned long v = std::stoul(p[2 + n1 + i]);
            if (v >= seen.size()) fail("invalid wire " + std::to_string(v) + " [0..." + std::to_string(seen.size()) + "[");
            seen[v] = true;
            outs.push_back((Wire)v);
        }
        const std::string &o = p.back();
        Operation op;
        size_t want = 2;
        if (o == "XOR") op = XOR;
        else if (o == "XNOR") op = XNOR;
        else if (o == "AND") op = AND;
        else if (o == "OR") op = OR;
        else if (o == "INV") {
            op = INV;
            want = 1;
        } else {
            fail("invalid operation '" + o + "'");
            op = XOR;
        }
        if (ins.size() != want) fail("invalid number of inputs " + std::to_string(ins.size()) + " for " + o);
        if (outs.size() != 1) fail("invalid number of outputs " + std::to_string(outs.size()) + " for " + o);
        c.Gates.push_back(Gate{ins[0], ins.size() > 1 ? ins[1] : 0, outs[0], op, 0});
    }
    if (gate != c.NumGates) fail("not enough gates: got " + std::to_string(gate) + ", expected " + std::to_string(c.NumGates));
    for (size_t i = 0; i < seen.size(); i++)
        if (!seen[i]) fail("wire " + std::to_string(i) + " not assigned");
    return c;
}

// circuit.Streaming (stream_garble.go:27-192); conn.WriteBuf becomes the caller's byte vector
class Streaming {
public:
    Streaming(Reader &rand, const std::vector<uint8_t> &key, const std::vector<Wire> &inputs,
              Context &ctx = Context::Default()) {
        std::vector<uint8_t> rnd(16 * (inputs.size() + 1));
        rand.Read(rnd.data(), 16);
        if (key.size() != 16 && key.size() != 24 && key.size() != 32)
            throw Error("crypto/aes: invalid key size " + std::to_string(key.size()));
        rand.Read(rnd.data() + 16, 16 * inputs.size());
        int st = GC_OK;
        h_ = gc_stream_create(ctx.handle(), key.data(), key.size(), rnd.data(), rnd.size(), inputs.data(),
                              (uint32_t)inputs.size(), &st);
        check(st, "gc_stream_create");
    }
    ~Streaming() { gc_stream_free(h_); }
    ot::Wire GetInput(Wire w) {
        ot::Wire out;
        check(gc_stream_get_wire(h_, w, (gc_wire *)&out), "gc_stream_get_wire");
        return out;
    }
    // Garble (stream_garble.go:161): appends the serialised gates to buf (conn.WriteBuf)
    void Garble(Circuit &c, const std::vector<Wire> &in, const std::vector<Wire> &out, std::vector<uint8_t> &buf) {
        size_t need = 0;
        const size_t at = buf.size();
        buf.resize(at + c.Gates.size() * 61 + 16);
        check(gc_stream_garble(h_, (const gc_gate *)c.Gates.data(), (uint32_t)c.Gates.size(), (uint32_t)c.NumWires,
                               in.data(), (uint32_t)in.size(), out.data(), (uint32_t)out.size(), buf.data() + at,
                               buf.size() - at, &need),
              "gc_stream_garble");
        buf.resize(at + need);
    }

private:
    gc_stream *h_ = nullptr;
};

}  // namespace circuit

// The four rounds of the reference's sha2pc package for S sessions per call (sha2pc/garbler.go, evaluator.go, encoding.go;
// gcengine.h: gc_sha2pc_*), on packed encoded payloads [S][len].  A check of the reference that a session fails is reported
// in verdict[s] (GC_SHA2PC_* | index << 8) with zero bytes for that session's outputs; the calls throw only for their own
// failures.  Randomness is the caller's, in the reference's consumption order.
namespace sha2pc {

struct Layout {
    size_t len[3], lead[3], digest_bytes;
};

inline Layout RoundLayout(const gc_circ *circ, uint32_t ng, uint32_t ne) {
    Layout l{};
    check(gc_sha2pc_layout(circ, ng, ne, l.len, l.lead, &l.digest_bytes), "gc_sha2pc_layout");
    return l;
}

// a bad session is the verdicts' to report
inline void check_round(int st, size_t bad, const char *what) {
    if ((st == GC_E_ARG || st == GC_E_POINT) && bad != (size_t)-1) return;
    check(st, what);
}

class GarblerBatch {
public:
    GarblerBatch(Context &ctx, gc_circ *circ, uint32_t ng, uint32_t ne, size_t S) : S_(S), l_(RoundLayout(circ, ng, ne)) {
        int st = GC_OK;
        h_ = gc_sha2pc_garbler_create(ctx.handle(), circ, ng, ne, S, &st);
        check(st, "gc_sha2pc_garbler_create");
    }
    ~GarblerBatch() { gc_sha2pc_garbler_free(h_); }
    GarblerBatch(const GarblerBatch &) = delete;
    GarblerBatch &operator=(const GarblerBatch &) = delete;
    const Layout &layout() const { return l_; }
    gc_sha2pc_garbler *handle() { return h_; }
    // GarblerRound1 + EncodeRound1: a [S][32], sid [S][8] -> A, AaInv [S], r1 [S][80]
    void Round1(const uint8_t *a, const uint8_t *sid, std::vector<gc_p256_point> &A, std::vector<gc_p256_point> &AaInv,
                std::vector<uint8_t> &r1, std::vector<uint32_t> &verdict) {
        A.resize(S_), AaInv.resize(S_), r1.resize(S_ * l_.len[0]), verdict.resize(S_);
        size_t bad = (size_t)-1;
        check_round(gc_sha2pc_garbler_round1(h_, a, sid, A.data(), AaInv.data(), r1.data(), verdict.data(), &bad), bad,
                    "gc_sha2pc_garbler_round1");
    }
    // DecodeRound2 + GarblerRound3 + EncodeRound3
    void Round3(const uint8_t *a, const gc_p256_point *AaInv, const uint8_t *sid, const uint8_t *r2, const uint8_t *keys,
                const uint8_t *rnd, const uint8_t *bits, std::vector<uint8_t> &r3, std::vector<uint32_t> &verdict) {
        r3.resize(S_ * l_.len[2]), verdict.resize(S_);
        size_t bad = (size_t)-1;
        check_round(gc_sha2pc_garbler_round3(h_, a, AaInv, sid, r2, keys, rnd, bits, r3.data(), verdict.data(), &bad), bad,
                    "gc_sha2pc_garbler_round3");
    }

private:
    gc_sha2pc_garbler *h_ = nullptr;
    size_t S_;
    Layout l_;
};

class EvaluatorBatch {
public:
    EvaluatorBatch(Context &ctx, gc_circ *circ, uint32_t ng, uint32_t ne, size_t S) : S_(S), l_(RoundLayout(circ, ng, ne)) {
        int st = GC_OK;
        h_ = gc_sha2pc_evaluator_create(ctx.handle(), circ, ng, ne, S, &st);
        check(st, "gc_sha2pc_evaluator_create");
    }
    ~EvaluatorBatch() { gc_sha2pc_evaluator_free(h_); }
    EvaluatorBatch(const EvaluatorBatch &) = delete;
    EvaluatorBatch &operator=(const EvaluatorBatch &) = delete;
    const Layout &layout() const { return l_; }
    gc_sha2pc_evaluator *handle() { return h_; }
    // DecodeRound1 + EvaluatorRound2 + EncodeRound2: scalars [S][ne][32], bits [S][ne] -> A [S], sid [S][8], r2 [S][len]
    void Round2(const uint8_t *r1, const uint8_t *scalars, const uint8_t *bits, std::vector<gc_p256_point> &A,
                std::vector<uint8_t> &sid, std::vector<uint8_t> &r2, std::vector<uint32_t> &verdict) {
        A.resize(S_), sid.resize(S_ * 8), r2.resize(S_ * l_.len[1]), verdict.resize(S_);
        size_t bad = (size_t)-1;
        check_round(gc_sha2pc_evaluator_round2(h_, r1, scalars, bits, A.data(), sid.data(), r2.data(), verdict.data(), &bad),
                    bad, "gc_sha2pc_evaluator_round2");
    }
    // DecodeRound3 + EvaluatorRound4 -> digests [S][digest_bytes]
    void Round4(const gc_p256_point *A, const uint8_t *sid, const uint8_t *scalars, const uint8_t *bits, const uint8_t *r3,
                std::vector<uint8_t> &digests, std::vector<uint32_t> &verdict) {
        digests.resize(S_ * l_.digest_bytes), verdict.resize(S_);
        size_t bad = (size_t)-1;
        check_round(gc_sha2pc_evaluator_round4(h_, A, sid, scalars, bits, r3, digests.data(), verdict.data(), &bad), bad,
                    "gc_sha2pc_evaluator_round4");
    }

private:
    gc_sha2pc_evaluator *h_ = nullptr;
    size_t S_;
    Layout l_;
};

}  // namespace sha2pc

// circuit.Garbler / circuit.Evaluator for S sessions of one circuit per call (circuit/garbler.go:38-180, evaluator.go:20-157;
// gcengine.h: gc_yao_*), on packed messages [S][len].  The OT between Send and Result is the caller's (mpc::ot, on the wires
// of OtWires).  A check that a session fails is reported in verdict[s] (GC_YAO_* | index << 8) with zero bytes for that
// session's outputs; the calls throw only for their own failures.
namespace yao {

struct Layout {
    size_t len[3];  // M1, M2, M3's slot
    size_t bits_bytes() const { return len[2] - 4; }
};

inline Layout MessageLayout(const gc_circ *circ, uint32_t ng, uint32_t ne, size_t keylen) {
    Layout l{};
    check(gc_yao_layout(circ, ng, ne, keylen, l.len), "gc_yao_layout");
    return l;
}

// a bad session is the verdicts' to report
inline void check_call(int st, size_t bad, const char *what) {
    if ((st == GC_E_ARG || st == GC_E_ROWS) && bad != (size_t)-1) return;
    check(st, what);
}

class GarblerBatch {
public:
    GarblerBatch(Context &ctx, gc_circ *circ, uint32_t ng, uint32_t ne, size_t keylen, size_t S)
        : S_(S), ne_(ne), l_(MessageLayout(circ, ng, ne, keylen)) {
        int st = GC_OK;
        h_ = gc_yao_garbler_create(ctx.handle(), circ, ng, ne, keylen, S, &st);
        check(st, "gc_yao_garbler_create");
    }
    ~GarblerBatch() { gc_yao_garbler_free(h_); }
    GarblerBatch(const GarblerBatch &) = delete;
    GarblerBatch &operator=(const GarblerBatch &) = delete;
    const Layout &layout() const { return l_; }
    gc_yao_garbler *handle() { return h_; }
    // Garble and the messages before the OT: keys [S][keylen], rnd [S][16 (1 + ng + ne)], bits [S][ng] -> m1 [S][len1]
    void Send(const uint8_t *keys, const uint8_t *rnd, const uint8_t *bits, std::vector<uint8_t> &m1) {
        m1.resize(S_ * l_.len[0]);
        check(gc_yao_garbler_send(h_, keys, rnd, bits, m1.data()), "gc_yao_garbler_send");
    }
    // garbled.Wires[offset : offset + count] of every session, session-major
    void OtWires(std::vector<gc_wire> &wires) {
        wires.resize(S_ * ne_);
        check(gc_yao_garbler_ot_wires(h_, wires.data()), "gc_yao_garbler_ot_wires");
    }
    // m2 [S][16 nout] -> m3 [S][4 + bits_bytes] (4 + n bytes used: len3 [S]), bits [S][bits_bytes]
    void Result(const uint8_t *m2, std::vector<uint8_t> &m3, std::vector<uint32_t> &len3, std::vector<uint8_t> &bits,
                std::vector<uint32_t> &verdict) {
        m3.resize(S_ * l_.len[2]), len3.resize(S_), bits.resize(S_ * l_.bits_bytes()), verdict.resize(S_);
        size_t bad = (size_t)-1;
        check_call(gc_yao_garbler_result(h_, m2, m3.data(), len3.data(), bits.data(), verdict.data(), &bad), bad,
                   "gc_yao_garbler_result");
    }

private:
    gc_yao_garbler *h_ = nullptr;
    size_t S_, ne_;
    Layout l_;
};

class EvaluatorBatch {
public:
    EvaluatorBatch(Context &ctx, gc_circ *circ, uint32_t ng, uint32_t ne, size_t keylen, size_t S)
        : S_(S), l_(MessageLayout(circ, ng, ne, keylen)) {
        int st = GC_OK;
        h_ = gc_yao_evaluator_create(ctx.handle(), circ, ng, ne, keylen, S, &st);
        check(st, "gc_yao_evaluator_create");
    }
    ~EvaluatorBatch() { gc_yao_evaluator_free(h_); }
    EvaluatorBatch(const EvaluatorBatch &) = delete;
    EvaluatorBatch &operator=(const EvaluatorBatch &) = delete;
    const Layout &layout() const { return l_; }
    gc_yao_evaluator *handle() { return h_; }
    // m1 [S][len1]: key, tables and the garbler's labels into the handle
    void Accept(const uint8_t *m1, std::vector<uint32_t> &verdict) {
        verdict.resize(S_);
        size_t bad = (size_t)-1;
        check_call(gc_yao_evaluator_accept(h_, m1, verdict.data(), &bad), bad, "gc_yao_evaluator_accept");
    }
    // labels [S][ne] from the OT -> m2 [S][16 nout]
    void Eval(const gc_label *labels, std::vector<uint8_t> &m2, std::vector<uint32_t> &verdict) {
        m2.resize(S_ * l_.len[1]), verdict.resize(S_);
        size_t bad = (size_t)-1;
        check_call(gc_yao_evaluator_eval(h_, labels, m2.data(), verdict.data(), &bad), bad, "gc_yao_evaluator_eval");
    }
    // m3 [S][4 + bits_bytes] -> bits [S][bits_bytes]
    void Result(const uint8_t *m3, std::vector<uint8_t> &bits, std::vector<uint32_t> &verdict) {
        bits.resize(S_ * l_.bits_bytes()), verdict.resize(S_);
        size_t bad = (size_t)-1;
        check_call(gc_yao_evaluator_result(h_, m3, bits.data(), verdict.data(), &bad), bad, "gc_yao_evaluator_result");
    }

private:
    gc_yao_evaluator *h_ = nullptr;
    size_t S_;
    Layout l_;
};

}  // namespace yao

// The random streams of S sessions, expanded on the device (gcengine.h: gc_rand_*): stream s is what a Go host reads from
// cipher.StreamReader{S: cipher.NewCTR(aes.NewCipher(seed[s]), iv[s]), R: zeros}, the reader it would set as env.Config.Rand.
// One byte position for all streams; every draw is one launch on the ctx stream.  The cursor calls (SetCursors, FillAt, Ints)
// keep one position per session in a device array of the caller's, advance it on the device and may be captured.
namespace rand {

class DeviceRand {
public:
    // seeds [S][keylen] (16 / 24 / 32), ivs [S][16] or nullptr for all-zero IVs
    DeviceRand(Context &ctx, const uint8_t *seeds, size_t keylen, const uint8_t *ivs, size_t S) : S_(S) {
        int st = GC_OK;
        h_ = gc_rand_create(ctx.handle(), seeds, keylen, ivs, S, &st);
        check(st, "gc_rand_create");
    }
    // device arrays, read behind what is queued on the ctx stream
    static DeviceRand FromDevice(Context &ctx, const void *d_seeds, size_t keylen, const void *d_ivs, size_t S) {
        int st = GC_OK;
        gc_rand *h = gc_rand_create_dev(ctx.handle(), d_seeds, keylen, d_ivs, S, &st);
        check(st, "gc_rand_create_dev");
        return DeviceRand(h, S);
    }
    ~DeviceRand() { gc_rand_free(h_); }
    DeviceRand(const DeviceRand &) = delete;
    DeviceRand &operator=(const DeviceRand &) = delete;
    DeviceRand(DeviceRand &&o) noexcept : h_(o.h_), S_(o.S_) { o.h_ = nullptr; }
    gc_rand *handle() { return h_; }
    size_t Sessions() const { return S_; }
    uint64_t Pos() const {
        uint64_t pos = 0;
        check(gc_rand_info(h_, nullptr, nullptr, &pos), "gc_rand_info");
        return pos;
    }
    void Seek(uint64_t pos) { check(gc_rand_seek(h_, pos), "gc_rand_seek"); }
    // the next nbytes of stream s to d_out + s * stride
    void Fill(size_t nbytes, void *d_out, size_t stride) { check(gc_rand_fill_dev(h_, nbytes, d_out, stride), "gc_rand_fill_dev"); }
    // the same into host memory: [S][nbytes]
    std::vector<uint8_t> FillHost(size_t nbytes) {
        std::vector<uint8_t> out(S_ * nbytes);
        check(gc_rand_fill(h_, nbytes, out.data(), nbytes), "gc_rand_fill");
        return out;
    }
    // circuit.Garbler's order (circuit/garbler.go:47-53): the key, then R and the input labels: d_keys [S][32] and d_rnd
    // [S][1 + ninputs][16] as circuit::GarbleBatchKeys takes them
    void DrawGarbler(uint32_t ninputs, void *d_keys, void *d_rnd) {
        Fill(32, d_keys, 32);
        Fill(16 * (size_t)(1 + ninputs), d_rnd, 16 * (size_t)(1 + ninputs));
    }
    // tripleBatch's draws (gmw/triples.go:301-310): a, b u64 [S][words]
    void GMWShares(size_t words, void *d_a, void *d_b) { check(gc_rand_gmw_shares_dev(h_, words, d_a, d_b), "gc_rand_gmw_shares_dev"); }

    // Per-session cursors: d_cur u64 [S] (8-byte aligned), d_status u64 [2] = {bad sessions, lowest bad session}.  A bad
    // session keeps its outputs and its cursor untouched.
    void SetCursors(void *d_cur, uint64_t pos) { check(gc_rand_cur_set_dev(h_, d_cur, pos), "gc_rand_cur_set_dev"); }
    // bytes [cur[s], cur[s] + nbytes) of stream s to d_out + s * stride; cur[s] += nbytes
    void FillAt(void *d_cur, size_t nbytes, void *d_out, size_t stride, void *d_status) {
        check(gc_rand_fill_cur_dev(h_, d_cur, nbytes, d_out, stride, d_status), "gc_rand_fill_cur_dev");
    }
    // `count` crand.Int(reader_s, max) draws per session, max 32 bytes big-endian: d_out [S][count][32] as
    // gc_co_multi_sender_setup_dev (count = 1) and gc_co_multi_receiver_choices_dev take their scalars
    void Ints(void *d_cur, const uint8_t max[32], size_t count, void *d_out, void *d_status) {
        check(gc_rand_scalars_cur_dev(h_, d_cur, max, count, d_out, d_status), "gc_rand_scalars_cur_dev");
    }
    // the host forms: cur [S] is read and written back; false and *bad_session = the lowest bad session when one is bad
    // (the good ones are written and advanced all the same)
    bool FillAtHost(uint64_t *cur, size_t nbytes, uint8_t *out, size_t stride, size_t *bad_session = nullptr) {
        size_t bad = (size_t)-1;
        return host_form(gc_rand_fill_cur(h_, cur, nbytes, out, stride, &bad), bad, bad_session, "gc_rand_fill_cur");
    }
    bool IntsHost(uint64_t *cur, const uint8_t max[32], size_t count, uint8_t *out, size_t *bad_session = nullptr) {
        size_t bad = (size_t)-1;
        return host_form(gc_rand_scalars_cur(h_, cur, max, count, out, &bad), bad, bad_session, "gc_rand_scalars_cur");
    }

private:
    static bool host_form(int st, size_t bad, size_t *bad_session, const char *what) {
        if (st == GC_E_ARG && bad != (size_t)-1) {
            if (bad_session) *bad_session = bad;
            return false;
        }
        check(st, what);
        return true;
    }
    DeviceRand(gc_rand *h, size_t S) : h_(h), S_(S) {}
    gc_rand *h_ = nullptr;
    size_t S_ = 0;
};

}  // namespace rand
}  // namespace mpc
