// Command-line driver with the reference's interface (src/main.cpp:145-159):
//     virgo_plus_run <file.pws> [--blocks B] [--batched | --fs] [--seed S] [--device D] [--dump transcript.bin]
//     --fs: non-interactive GKR proof (Fiat-Shamir over SHA3-256), then verified from the proof bytes alone
//     --record FILE: (interactive mode with the commitment) writes the record of the run — everything the prover handed over, layout in vphost.h;
//         its query phase is then answered in one device pass (verifier::batched_openings)
//     virgo_plus_run --check-record FILE <file.pws> [--blocks B] [--seed S]: verifies such a record with the host verifier alone, no GPU
//         --device-verifier [--device D]: the same replay with the verifier's heavy loops (wiring predicates, public polynomial values, opening
//         digests) on GPU D, as vph_verify_full_record_dev runs it; the comparisons and the verdict stay on the host
// Loads the circuit, runs the GKR proof on the GPU against the host verifier and prints the
// reference's result lines (interactive mode runs the whole protocol incl. the Virgo commitment and its verification).
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "circuit.hpp"
#include "prover.hpp"
#include "verifier.hpp"

int main(int argc, char **argv) {
    if (argc < 2) { fprintf(stderr, "usage: %s <file.pws> [--blocks B] [--batched | --fs | --fs-device] [--device D] [--dump out.bin]\n", argv[0]); return 2; }
    int blocks = 1, device = 0; bool batched = false, fsmode = false, fs_device = false; const char *dump = nullptr, *record = nullptr, *check_record = nullptr;
    bool device_verifier = false;
    int first = 2;
    if (!strcmp(argv[1], "--check-record")) {
        if (argc < 4) { fprintf(stderr, "usage: %s --check-record record.bin <file.pws> [--blocks B] [--seed S]\n", argv[0]); return 2; }
        check_record = argv[2]; argv[1] = argv[3]; first = 4;
    }
    for (int i = first; i < argc; ++i) {
        std::string a = argv[i];
        if (a == "--blocks" && i + 1 < argc) blocks = atoi(argv[++i]);
        else if (a == "--device" && i + 1 < argc) device = atoi(argv[++i]);
        else if (a == "--batched") batched = true;
        else if (a == "--fs") fsmode = true;
        else if (a == "--fs-device") fsmode = fs_device = true;      // the same proof with every challenge drawn on the device (verifier::proveFSDevice)
        else if (a == "--device-verifier" && check_record) device_verifier = true;
        else if (a == "--seed" && i + 1 < argc) srandom((unsigned) atol(argv[++i]));      // witness draw (default: glibc's initial state, as the reference)
        else if (a == "--dump" && i + 1 < argc) dump = argv[++i];
        else if (a == "--record" && i + 1 < argc) record = argv[++i];
        else { fprintf(stderr, "bad argument %s\n", argv[i]); return 2; }
    }
    std::vector<DAG_gate> dag;
    std::string err;
    if (!vph::parse_pws(argv[1], blocks, dag, &err)) { fprintf(stderr, "%s\n", err.c_str()); return 2; }
    layeredCircuit c = vph::DAG_to_layered(dag);
    F::init();
    c.subsetInit();
    if (check_record) {                              // the host verifier alone: same generator state as the run that wrote the record
        std::vector<uint8_t> rec;
        FILE *f = fopen(check_record, "rb");
        if (!f) { fprintf(stderr, "cannot read %s\n", check_record); return 2; }
        uint8_t buf[65536];
        for (size_t k; (k = fread(buf, 1, sizeof buf, f)) > 0;) rec.insert(rec.end(), buf, buf + k);
        fclose(f);
        bool ok = false;
        if (device_verifier) {
            try { ok = checkFullOnDevice(c, device, rec); } catch (const std::exception &e) { fprintf(stderr, "%s\n", e.what()); return 2; }
        } else {
            try { verifier v(nullptr, c); ok = v.checkFull(rec); } catch (const std::exception &) { ok = false; }
        }
        if (!ok) { fprintf(stderr, "Verification fail\n"); return 1; }
        fprintf(stderr, "Verification pass\n");
        return 0;
    }
    if (record && (batched || fsmode || c.circuit[0].bitLength < 7)) { fprintf(stderr, "--record needs the interactive mode and an input layer of at least 2^7 wires\n"); return 2; }
    try {
        prover p(c, device);
        bool ok;
        std::vector<uint8_t> tr;
        double vt = 0, pc_pt = -1;
        if (fsmode) {
            verifier v(&p, c);
            ok = fs_device ? (v.proveFSDevice(), true) : v.proveFS();
            tr = v.transcript();
            verifier w(nullptr, c);                  // a verifier that has only the proof
            ok = ok && w.checkFS(tr);
            vt = w.verifyTime();
            batched = true;                          // report the proof's own size
        } else if (batched) {
            verifier v(nullptr, c);
            std::vector<F> tape = v.drawTape();
            p.proveGKR(tape, tr);
            ok = v.check(tape, tr);
            vt = v.verifyTime();
        } else if (c.circuit[0].bitLength >= 7) {
            verifier v(&p, c);                       // the reference's flow: commitment on (src/verifier.cpp:134-189)
            v.batched_openings = record != nullptr;
            ok = v.verifyFull();
            tr = v.fullTranscript();
            if (ok && record) {
                FILE *f = fopen(record, "wb");
                if (!f || fwrite(v.fullRecord().data(), 1, v.fullRecord().size(), f) != v.fullRecord().size()) { fprintf(stderr, "cannot write %s\n", record); if (f) fclose(f); return 2; }
                fclose(f);
            }
            vt = v.verifyTime() + v.polyVerifyTime();
            pc_pt = v.polyProveTime();
        } else {
            verifier v(&p, c);
            ok = v.verify();
            tr = v.transcript();
            vt = v.verifyTime();
        }
        if (!ok) { fprintf(stderr, "Verification fail\n"); return 1; }
        fprintf(stderr, "Verification pass\n");
        fprintf(stdout, "Input size %d\n", (int) c.circuit[0].size);
        fprintf(stdout, "Prove Time %lf\n", p.proveTime());
        fprintf(stdout, "verify time %lf\n", vt);
        fprintf(stdout, "proof size = %lf kb\n", batched ? tr.size() / 1024.0 : p.proofSize());
        if (pc_pt >= 0) fprintf(stdout, "Polynomial commitment: prove time %lf\n", pc_pt);
        if (dump) { FILE *f = fopen(dump, "wb"); if (f) { fwrite(tr.data(), 1, tr.size(), f); fclose(f); } }
    } catch (const std::exception &e) {
        fprintf(stderr, "error: %s\n", e.what());
        return 3;
    }
    return 0;
}
