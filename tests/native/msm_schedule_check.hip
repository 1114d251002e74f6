// Stand-alone host program around the MSM launch schedule (co-zkvms_amd/csrc/host/msm_schedule.hpp): no device code runs, no GPU
// and no project library is needed.  Built by co-zkvms_amd/build.py and driven by tests/test_msm_schedule_host.py.
//
//   in  (text): per case one line  "case <nwin> <n_bases> <form> <shape_rule> <wg_digits_log2> <set_refs_log2> <serial> <ltpb> <wgs> <columns>"
//               (form: auto | plain | offset; ltpb / wgs: a number, or - for "not overridden"), then <columns> lines "<kind> <offset> <n>"
//   out (text): per case "CASE <number>", then either "REFUSED <text>" or one line per launch set in launch order: the
//               COZK_TRACE_MSM line followed by " | block b groups g pipelined 0|1 cols first G g nb x bound x L0 x maxseg0 x
//               fold x part x exc x blk x ws w elig hex force 0|1"
// The options come from the case, never from this process's environment.
#include <iostream>
#include <sstream>
#include <string>
#include <vector>
#include "../../co-zkvms_amd/csrc/host/msm_schedule.hpp"

static int kind_of(const std::string& name) {
    for (int kind = 0; kind < MSM_KINDS; kind++)
        if (name == MSM_KIND_NAME[kind]) return kind;
    return -1;
}
static int override_of(const std::string& word) { return word == "-" ? MSM_BY_SHAPE : atoi(word.c_str()); }

int main() {
    std::string word, form, ltpb, wgs;
    for (int number = 0; std::cin >> word; number++) {
        if (word != "case") return 2;
        int nwin = 0, shape_rule = 1, serial = 0;
        size_t n_bases = 0, k = 0;
        MsmOptions o;
        if (!(std::cin >> nwin >> n_bases >> form >> shape_rule >> o.wg_digits_log2 >> o.set_refs_log2 >> serial >> ltpb >> wgs >> k)) return 2;
        o.shape_rule = shape_rule != 0;
        o.serial = serial != 0;
        o.ltpb = override_of(ltpb);
        o.wgs = override_of(wgs);
        std::vector<size_t> offsets(k), ns(k);
        std::vector<int> kinds(k);
        std::vector<uint8_t> elig(k);
        for (size_t p = 0; p < k; p++) {
            if (!(std::cin >> word >> offsets[p] >> ns[p])) return 2;
            kinds[p] = kind_of(word);
        }
        std::ostringstream out;
        try {
            o.digit_form = msm_digit_form_parse(form.c_str());
            msm_options_check(o);
            for (size_t p = 0; p < k; p++) elig[p] = msm_column_eligible(nwin, o, kinds[p], ns[p]);
            const MsmBatchSchedule sched = msm_schedule(nwin, n_bases, offsets.data(), ns.data(), kinds.data(), k, elig.data(), o);
            for (size_t b = 0; b < sched.blocks.size(); b++)
                for (const MsmSetSchedule& s : sched.blocks[b].sets)
                    out << msm_set_trace_line(s) << " | block " << b << " groups " << sched.blocks[b].ngroups << " pipelined " << sched.blocks[b].pipelined
                        << " cols " << s.first << " G " << s.G << " nb " << s.nb << " bound " << s.bound << " L0 " << s.L0 << " maxseg0 " << s.maxseg0
                        << " fold " << s.fold_levels << " part " << s.part_entries << " exc " << s.exc_entries << " blk " << s.blk_entries << " ws " << s.ws
                        << " elig " << std::hex << s.elig << std::dec << " force " << s.force_offset << "\n";
        } catch (const CozkError& e) {
            out.str("");
            out << "REFUSED " << e.what() << "\n";
        }
        std::cout << "CASE " << number << "\n" << out.str();
    }
    return std::cout.flush() ? 0 : 4;
}
