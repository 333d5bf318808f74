"""The cgo shim of the VOLE (go/vole/vole_hip.go) is source only (no Go toolchain in the image): it must be a gchip build,
indented with tabs, call the two host entry points of the VOLE section, keep the reference's IKNP calls, messages and
error strings (vole/vole.go), and keep a math/big path for the moduli the ABI refuses.  tests/test_abi_plan.py checks its
C calls against the prototypes with every other shim."""
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHIM = os.path.join(ROOT, "go", "vole", "vole_hip.go")

# the error strings of vole.go's two Mul bodies, which a Go caller may match on
ERRORS = [
    "vole: ExpandSend: %w", "vole: ExpandSend returned %d wires, want %d", "vole: MulSender receive y-vector: %w",
    "vole: MulSender expected %d bytes for y-vector, got %d", "vole: MulSender send u-vector: %w",
    "vole: MulSender flush u-vector: %w", "vole: nil Ext", "vole: ExpandReceive: %w",
    "vole: ExpandReceive returned %d labels, want %d", "vole: MulReceiver send y-vector: %w",
    "vole: MulReceiver flush y-vector: %w", "vole: MulReceiver receive u-vector: %w",
    "vole: MulReceiver expected %d bytes for u-vector, got %d",
]


def test_vole_shim_calls_the_vole_entry_points():
    text = open(SHIM).read()
    assert text.startswith("//go:build gchip")
    assert "\n    " not in text.replace("\n    //", ""), "indent with tabs (gofmt)"
    assert re.search(r"^package vole$", text, re.M)
    calls = set(re.findall(r"\bC\.(gc_[a-z0-9_]+)\(", text))
    assert {"gc_vole_sender_mul", "gc_vole_receiver_reduce"} <= calls, calls
    hdr = open(os.path.join(ROOT, "include", "gcengine.h")).read()
    for name in calls:
        assert re.search(r"\b%s\s*\(" % name, hdr), name


def test_vole_shim_keeps_the_reference_around_the_calls():
    text = open(SHIM).read()
    for e in ERRORS:
        assert '"%s"' % e in text, e
    assert "e.iknp.Send(m, false)" in text and "e.iknp.Receive(flags, labels, false)" in text
    assert text.count("e.conn.SendData(") == 2 and text.count("e.conn.ReceiveData()") == 2 and text.count("e.conn.Flush()") == 2
    assert "bytes32(inputs[i])" in text  # the receiver's y-message is built exactly as Go builds it
    # the refused moduli keep the reference's math/big loops
    assert "prgExpandLabel(ld, &pad)" in text and "us[i].Mod(us[i], p)" in text
