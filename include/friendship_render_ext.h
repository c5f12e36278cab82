/*
 * friendship_render_ext.h -- entry points of the MI355X engine beyond the drop-in boundary of friendship_render.h.
 *
 * friendship_render.h is the symbol set every renderer library exports (the product and the CPU oracle alike).  What is
 * declared here only the product exports: a host that loads a renderer library at run time resolves these with dlsym and
 * copes with their absence (libfriendship_amd/host/friendship.hpp PluginRenderer, libfriendship_amd/capi.py).
 */
#ifndef FRIENDSHIP_RENDER_EXT_H
#define FRIENDSHIP_RENDER_EXT_H

#include "friendship_render.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ---- per-renderer options --------------------------------------------------------------------
 * Every tuning switch of the engine is named like the environment variable that sets it for the whole process
 * (INTEGRATION.md §5), and its value string means what it means in the environment.  Most of them can also be given to
 * one renderer when it is created, so that two renderers of one process (a real-time instance with short blocks next to
 * an offline bounce) can differ.  Precedence: an option beats the environment, the environment beats the built-in
 * default.  Everything is read once, when the renderer is created.
 *
 * Options are checked strictly: an unknown name, a name that is process-wide only (FR_JIT_CACHE, FR_JIT_DUMP,
 * FR_HOST_TRACE, FR_LOWER_TRACE, FR_PLAN_TRACE, FR_LOWER_HUGEPAGES), a name given twice, a value that does not parse
 * (decimal digits, or a word the switch documents such as "force") or is out of range: FR_ERR_INVALID_ARG and no
 * renderer.  (The environment keeps its lenient reading: atoi and clamping, as always.)
 *
 * FR_RING_KEEP = 0 / 1 (default 0; read strictly from the environment too): kept delay lines.  A graph edit, a finished
 * run-time compile or a call longer than any before makes the renderer re-plan; without the option the first call of the
 * new plan re-renders the look-back window of every delay line, and a plan with feedback loops replays every frame since 0.
 * With it, delay lines whose contents the edit cannot have changed (same lowered node, same loops, enough frames held)
 * are kept -- moved to their new place on the device if the plan renumbers them -- and only the others are rebuilt
 * before the call.  Results are the same bits.  fr_plan_json: "ring_keep", and per call "ring_state" {kept, rebuilt, moved,
 * move_launches, repair_from, inert}; launches of form "repair" / "replay" in bank_launches and stage_launches.  The option
 * does nothing ("inert" names why) under FR_SHARD_PARTIALS, with a track history that feeds delay lines, and with a
 * bounded input history (fr_config.history_frames).
 *
 * FR_STREAM_PROGRAMS = 0 / 1 (default 0; read strictly from the environment too): block streaming (fr_stream_begin /
 * fr_stream_block / fr_stream_end, friendship_render.h) also serves plans with stage programs and delay lines behind one
 * bank of balanced template voices: a second resident kernel runs each voice's programs in the wave that finishes the voice.
 * With 0 nothing changes: the same plans are served and refused, by the same kernel.  With 1, fr_plan_json carries "stream"
 * {servable, reason, voices, chunks, programs_per_voice, min_ring_delay, rings, kernel} after any call: whether
 * fr_stream_begin would take the plan and why not.  Refused (FR_ERR_UNSUPPORTED, the reason in fr_last_error): a Delay of a
 * computed value shorter than 64 frames, a program that needs two voices of the same block (a mix bus), delayed reads of
 * the input row, signal-amount delays, more than one bank, compiled, general and track voices, pull rows, sharding.
 *
 * FR_STREAM_BUS = 0 / 1 (default 0; read strictly from the environment too; does nothing unless FR_STREAM_PROGRAMS=1):
 * block streaming also serves mix-bus programs across voices -- several voices, each with its own gain, envelope or taps,
 * summed to a mono or stereo bus, with taps or an echo behind the bus.  A program that reads, less than 64 frames back, two or
 * more voices (or what an earlier bus program stored) is a bus program: a third resident kernel runs the bus programs in the
 * workgroup that counts the block's last voice in, before it reports the block done.  With 0 nothing changes: the same
 * plans are served and refused, with the same reasons, by the same kernels.  "stream" gains "bus_programs": how many
 * programs run after the last voice (programs_per_voice counts the others).  Still refused: a Delay shorter than 64 frames
 * of a value computed by the reading program itself or a later one (a short loop, a bus echo of 32 frames), and everything
 * else of the list above.
 *
 * FR_STREAM_INPUTS = 0 / 1 (default 0; read strictly from the environment too; does nothing unless FR_STREAM_PROGRAMS=1):
 * block streaming also serves plans whose programs read, at the current frame, input slots other than 0 -- control rows: a
 * gain per voice, a gate, a mod wheel, a master volume -- up to 8 distinct slots, slot 0 included, in per-voice and in bus
 * programs alike.  fr_stream_block_rows (below) hands in a block's rows; a fourth resident kernel takes all of them in one
 * look at the doorbell.  With 0 nothing changes: the same plans are served and refused, with the same reasons, by the same
 * kernels.  "stream" gains "input_slots": the slots whose rows the resident launch reads, slot 0 first, the others ascending
 * ([0] for a plan that reads nothing else); "kernel" is "bank_stream_in_kernel" exactly when a program reads another slot.
 * Still refused: more than 8 distinct slots, delayed reads of an input row (a stream keeps no input history), voices whose
 * time is not slot 0, and everything else of the lists above.
 *
 * FR_STREAM_BANKS = 0 / 1 (default 0; read strictly from the environment too; does nothing unless FR_STREAM_PROGRAMS=1):
 * block streaming also serves plans of 2 to 8 voice banks -- a chord whose notes have 1024, 256 and 128 partials, dry voices
 * that go straight to their rows next to enveloped voices on a bus -- with or without programs behind them.  A fifth
 * resident kernel takes the bank table as a launch argument; every bank gets its own chunk size, the largest chunk halved
 * first, so that the partials per workgroup even out.  It composes with FR_STREAM_BUS and FR_STREAM_INPUTS, which such a
 * patch needs as a one-bank patch does.  With 0 nothing changes: the same plans are served and refused, with the same
 * reasons, by the same kernels.  "stream" gains "banks" ({voices, partials, chunks, to_ring} per bank, in plan order),
 * "workgroups" and "max_workgroups"; for several banks "voices" is their total, "chunks" the largest per-voice count,
 * programs_per_voice runs over the voices bank by bank, and "kernel" is "bank_stream_banks_kernel" exactly when the plan has
 * more than one bank.  Still refused: more than 8 banks, more voices in total than workgroups, and for every bank what is
 * refused for one: general, compiled and track voices, voices under 128 partials, voices whose time is not slot 0.
 *
 * FR_LOOP_TILES = 0 / 1 (default 0; read strictly from the environment too): loop tiles.  Feedback through a Delay of at most
 * 16 frames ("max_stride" below) -- a one-pole filter, a DC blocker, a short comb -- is rendered by launches whose threads walk the frames of the
 * call in order; with the option, one wave per loop renders the call in tiles of up to 256 frames: all 64 lanes fetch the
 * tile's inputs into on-chip memory, one lane per residue of the stride computes the frames from there, all lanes store the
 * tile.  The steady call, the replay after a seek and the replay of FR_RING_KEEP take this form.  Results are the same bits.
 * The stride of a feedback plan becomes the gcd of its loops' own delays (a later stage's read of a loop's output at another
 * delay no longer shortens it).  fr_plan_json gains "loop_tiles" {frames, max_stride, reason} -- frames per tile, 0 with the
 * reason when the plan is not tiled: a stride above max_stride, a loop that reads its own ring further back than one stride
 * (taps at d and 2d), a program of more than 16 frame-only loads or 12 stores, a Delay of a signal amount -- the tiled
 * launches' "variant" carries +tile, and "stage_jit_form" gains "tile".  With the option unset nothing changes.
 *
 * FR_LOOP_DYN = 0 / 1 / 2 (default 0; read strictly from the environment too): feedback through a Delay of a SIGNAL amount --
 * a flanger with regeneration, a comb or plucked string with vibrato, a tape echo x = in + g Delay(x, base + depth lfo(t)).
 * With 0 such a cycle is FR_ERR_CYCLE as ever, every message, plan and kernel unchanged.  With 1 or 2 a cycle that has no Delay
 * of a constant >= 1 frames on it is cut at its innermost Delay of a signal amount, and the plan is served when interval
 * arithmetic over the amount's expression proves it never NaN, >= 1.0 and < 2^31; the bound in frames is floor(lo) of the
 * interval, which is widened outward at every step: 1 + lfo is NOT provable (lo falls below 1), 2 + lfo is, with bound 1, and
 * 8 + 6 Minimum(1, Modulo(In1 r, 1)) has bound 7, not 8.  An amount fed by a raw input row can be NaN: write the clamp as
 * Minimum(c, x) with the constant on the LEFT, which is free of NaN in both semantics.  Not provable: FR_ERR_CYCLE, the
 * message names the lowered node and the interval.  A signal tap of a delay line its own loop stores needs the same proof
 * (a bound of 0 frames there: FR_ERR_UNSUPPORTED); a tap behind the loop needs none.  Such a plan is a sweep plan: W, the
 * least bound of the loops' reads of their own delay lines, frames at a time are independent.  1 renders each level of loops in
 * ONE launch of stage_sweep_kernel (a workgroup per loop, min(W, 256) frames per sweep, a barrier between sweeps); 2 renders the
 * same programs through stage_kernel, one launch per W frames -- the cross-check and the baseline.  Same bits either way.  The
 * programs run on the interpreter (stage_jit_form null); FR_LOOP_TILES and FR_RING_KEEP are inert for a sweep plan (their reasons
 * say so), block streaming refuses it, FR_SHARD_PARTIALS, FR_MODE_PULL and history_frames refuse it as they refuse every
 * feedback plan.  Once set, fr_plan_json gains "loop_dyn" {sweep: W, frames: min(W, 256), form: "sweep" | "windows" | "",
 * reason}, and the launches' "variant" reads stage_sweep_kernel/feedback+sweep, stage_sweep_kernel/replay+sweep or
 * stage_kernel/windows.
 *
 * FR_STREAM_LOOPS = 0 / 1 (default 0; read strictly from the environment too; does nothing unless FR_STREAM_PROGRAMS=1):
 * block streaming also serves feedback loops shorter than a block -- y = a x + b Delay(y, 1), a comb or plucked string
 * x = voice + g Delay(x, d) with d < 64, a master filter or a 32-frame echo on a bus (with FR_STREAM_BUS) -- and what reads a
 * loop's output behind it on the same voice (a tap Delay(x, 2), a second row).  A program that reads, less than 64 frames
 * back, a delay line it stores itself is a loop program; its stride is the gcd of those delays.  A sixth resident kernel
 * (bank_stream_loops_kernel) runs it in the wave that finishes its voice: all lanes fetch the block's inputs into on-chip
 * memory, one lane per residue of the stride computes the frames from there in order, all lanes store the block.  It composes
 * with FR_STREAM_BUS, FR_STREAM_INPUTS and FR_STREAM_BANKS and does not depend on FR_LOOP_TILES.  With 0 nothing changes: the
 * same plans are served and refused, with the same reasons, by the same kernels.  "stream" gains "loop_programs" (the stride
 * of every streamed program in the order they run, voice by voice, then the bus programs; 0 for a program that is no loop),
 * "loop_loads" and "loop_stores" (the limits below); "kernel" is "bank_stream_loops_kernel" exactly when a program is a loop
 * program.  Still refused: a loop program of more than 32 loads (input rows and delay-line reads) or 16 stored delay lines
 * (the reason names the count and the limit), a Delay shorter than 64 frames of a computed value in a plan without a loop,
 * delayed reads of an input row, signal-amount delays, and everything else of the lists above.
 *
 * FR_STREAM_GENERAL = 0 / 1 (default 0; read strictly from the environment too; does nothing unless FR_STREAM_PROGRAMS=1):
 * block streaming also serves voices of ANY partial count and any tree of sums -- 24, 100, 300, 1000 partials, a chain, a
 * lopsided tree: what fr_fill_buffer renders as general voices -- and balanced voices of 32 or 64 partials.  Such a voice is
 * rendered by one workgroup of a seventh resident kernel (bank_stream_general_kernel), which runs the voice's schedule -- its
 * complete sub-trees of up to 2048 leaves, each split over up to 16 waves, then the sums above them -- exactly as the
 * ordinary path does: same bits.  Everything behind the voices (programs, FR_STREAM_BUS, FR_STREAM_INPUTS, FR_STREAM_LOOPS)
 * applies to such voices as to any other; next to voices of other sizes they need FR_STREAM_BANKS like any second bank.  With
 * 0 nothing changes: the same plans are served and refused, with the same reasons, by the same kernels.  "stream" gains
 * "general_voices" (the leaf count of every voice served this way, in voice order; [] when there is none) and
 * "general_max_leaves"; with FR_STREAM_BANKS the "banks" entries gain "general" (such a bank reports its largest voice as
 * "partials" and 1 chunk); "kernel" is "bank_stream_general_kernel" exactly when a voice is served this way.  Still refused:
 * a voice of more than 32768 leaves (one workgroup renders it; the reason names the count and the limit), more voices than
 * the device has compute units, compiled and track voices.
 *
 * FR_STREAM_DYN = 0 / 1 (default 0; read strictly from the environment too; does nothing unless FR_STREAM_PROGRAMS=1):
 * block streaming also serves a voice delayed by a SIGNAL amount -- a chorus, a flanger, a vibrato
 * (Delay(voice, base + depth * lfo(t))), a delay time on a knob (Delay(voice, Minimum(In(1), 48)), with FR_STREAM_INPUTS) --
 * and a constant delayed by a signal amount.  The planner's proven bound for the amount sizes the voice's delay line as in
 * fr_fill_buffer; an eighth resident kernel (bank_stream_dyn_kernel: the seventh's work with an interpreter that knows the
 * two ops) reads it with the reference's cast of the amount: same bits, in both semantics.  A delayed voice other than the
 * row's own makes the row a mix bus (FR_STREAM_BUS).  It composes with every option above.  With 0 nothing changes: the same
 * plans are served and refused, with the same reasons, by the same kernels.  "stream" gains "dyn_reads" and "dyn_steps" (the
 * streamed programs' signal delays of a voice and of a constant) and "lookback" (the deepest delay-line read, the bound
 * included); "kernel" is "bank_stream_dyn_kernel" exactly when there is such a delay.  Still refused, each with its reason: a
 * signal delay inside a feedback loop shorter than a block, of a computed value (a ring that a program stores), of an input
 * row (a stream keeps no input history; FR_STREAM_HISTORY below), and one whose bound was observed from input rows
 * (FR_DELAY_OBSERVED).
 *
 * FR_STREAM_HISTORY = 0 / 1 (default 0; read strictly from the environment too; does nothing unless FR_STREAM_PROGRAMS=1):
 * block streaming also serves a DELAYED READ OF AN INPUT ROW -- Delay(In(k), d): a pre-delay or a slap-back on a control or
 * audio row, a delayed gate, an LFO row read a quarter period late, Delay(In(0), d) on the time row itself -- at any constant
 * delay, 0..63 frames included, in per-voice programs, mix buses (FR_STREAM_BUS) and feedback loops shorter than a block
 * (FR_STREAM_LOOPS); and, with FR_STREAM_DYN, by a signal amount for which the planner proves a bound (Delay(In(1),
 * Minimum(In(2), 48))).  A slot other than 0 needs FR_STREAM_INPUTS as before and counts towards its 8 slots.  The stream
 * keeps a history of the rows it is fed -- the power of two >= the deepest such read + 64 frames per streamed slot, at most
 * 1 048 576 frames back (4 MiB per slot) -- in a ninth resident kernel (bank_stream_hist_kernel); a seek empties it, as a seek
 * of fr_fill_buffer makes every earlier input read 0.0: same bits, in both semantics.  With 0 nothing changes: the same plans
 * are served and refused, with the same reasons, by the same kernels.  "stream" gains "hist_reads" and "hist_dyn_reads" (the
 * streamed programs' delayed reads of input rows by a constant and by a signal amount) and "input_lookback" (the deepest of
 * them); "kernel" is "bank_stream_hist_kernel" exactly when there is such a read.  Still refused, each with its reason: a
 * signal delay of an input row without FR_STREAM_DYN, without a proven bound, inside a feedback loop shorter than a block, or
 * next to a bound observed from input rows; a read further back than the limit; a patch without a voice (FR_STREAM_EFFECTS
 * below).
 *
 * FR_STREAM_EFFECTS = 0 / 1 (default 0; read strictly from the environment too; does nothing unless FR_STREAM_PROGRAMS=1):
 * block streaming also serves a PATCH WITHOUT A VOICE -- no oscillator bank at all: an echo, a comb or a flanger on a row the
 * host feeds in, a gain or a minimum of two control rows, a one-pole smoother on a knob.  Its stage programs are dealt over
 * SEGMENTS, one workgroup of one wave each, in a tenth resident kernel (bank_stream_fx_kernel): every program gets a group in
 * the order the programs run; a program that reads an earlier program's delay line less than a block back (the tap behind a
 * loop, FR_STREAM_LOOPS) or copies it to a row follows that program's group; one that would follow two groups is a mix bus
 * (FR_STREAM_BUS) and runs after every segment has finished; group g runs in segment g mod segments, segments = min(groups,
 * the device's workgroups), so no patch is refused for its number of rows.  Every other rule applies to these programs as to a
 * voice's: slots other than 0 need FR_STREAM_INPUTS (slot 0 stays row 0 of every block), loops shorter than a block
 * FR_STREAM_LOOPS, delayed reads of input rows FR_STREAM_HISTORY, signal amounts FR_STREAM_DYN; same bits as fr_fill_buffer,
 * in both semantics.  With 0 nothing changes: such a patch is refused with "block streaming needs a plan with one voice bank
 * (this one: 0 bank launches)", and every other plan is served and refused, with the same reasons, by the same kernels.
 * "stream" gains "segments" (0 for a plan with voices); for a patch without a voice "voices" is 0, "programs_per_voice" lists
 * the programs of each segment and "kernel" is "bank_stream_fx_kernel".  Still refused, each with its reason: a patch with
 * neither voices nor programs; a feed-forward delay shorter than a block of a computed value (no fused form) and a signal
 * delay of one; a program that needs two groups without FR_STREAM_BUS.
 *
 * FR_STREAM_STORE = 0 / 1 (default 0; read strictly from the environment too; does nothing unless FR_STREAM_PROGRAMS=1): a
 * stream that SURVIVES EDITS.  The resident launch appends every row it is fed to the renderer's input store, under the
 * acknowledgement it already gives the rows (two more resident kernels, bank_stream_store_kernel and, for a patch without a
 * voice, bank_stream_store_fx_kernel: the top of the cascade and one vector store per streamed row more), and the renderer's
 * books follow block by block.  The contract of fr_stream_* becomes: results and statuses are those of fr_fill_buffer for
 * the same sequence of calls and edits, whatever mixture of fr_fill_buffer, edits and streams the host makes.
 *   - A stream's first block with idx == the renderer's next frame CONTINUES: the stream's history of its rows is filled from
 *     the store, the delay lines are brought up to idx as the first fr_fill_buffer call of the plan there would bring them before
 *     its own frames (nothing when that call would be steady, else the look-back rebuild from the stored history, a loop's
 *     replay, with FR_RING_KEEP its keep-and-repair), then the resident launch starts.  Any other idx is the seek it has always
 *     been, and resets the store as fr_fill_buffer's seek does.
 *   - Closing a stream (an edit, fr_fill_buffer*, fr_stream_end) leaves the renderer as after an ordinary call ending at the
 *     stream's last frame.  After an edit the host calls fr_stream_begin again and the first block continues.
 *   - Streamed are the slots the plan reads, every slot the store has been fed and every slot a block feeds, slot 0 first: at
 *     most 8, else fr_stream_begin (or the block) returns FR_ERR_UNSUPPORTED with the count and the limit and the renderer
 *     stays as it was -- go on with fr_fill_buffer, no seek needed.  Every servable plan takes this path, also one bank of
 *     balanced voices writing rows.
 *   - When a slot's buffer has to slide (fr_config.history_frames) or grow, or a block feeds a slot the launch does not
 *     stream, the launch is stopped, the store does what it does for fr_fill_buffer, and the launch restarts at the block:
 *     a relaunch, not a seek -- delay lines and history stay.  It costs a launch, once per ~65 000 frames with a bounded history
 *     and at every doubling (2^20, 2^21 ... frames) without.
 *   - FR_ERR_INPUT_HISTORY and FR_ERR_INPUT_TOO_LONG across every boundary are fr_fill_buffer's for the same sequence.
 * Inert -- the stream behaves as without the option, and "store"."inert" says why -- with FR_DELAY_OBSERVED=1 (streamed rows
 * would escape the observed bounds) and with declared track slots (fr_set_track_inputs).  With 0 nothing changes: not a plan,
 * not a kernel choice, not a status, not a bit.  "stream" gains "store": {"on", "slots" (the slots such a stream streams),
 * "continued" (the open stream's first block continued the store), "relaunches" (since fr_stream_begin), "inert"}, and
 * "kernel" names the two new kernels.
 *
 * FR_STREAM_TAPS = 0 / 1 (default 0; read strictly from the environment too; does nothing unless FR_STREAM_PROGRAMS=1): block
 * streaming also serves SHORT AND SIGNAL DELAYS OF COMPUTED VALUES in a patch without feedback -- "envelope, then effect":
 * e = env * voice, y = e + 0.5 * Delay(e, 1) (a two-tap low-pass behind an envelope); a chorus behind the ADSR or one chorus on the
 * mix bus (Delay(e, 40 + 30 * lfo(t)), with FR_STREAM_DYN); FIR stages behind a bus (FR_STREAM_BUS); Delay(In(1) * In(2), 10) in a
 * patch without a voice (FR_STREAM_EFFECTS).  Such a plan has no one-launch form for fr_fill_buffer either: it runs level by
 * level.  The stream runs the same levels, in order, inside its one resident launch and adds no kernel: a program that reads,
 * fewer than 64 frames back (0 included) or by a signal amount, a delay line that an earlier program stores runs behind that
 * program in the same voice's wave (a patch without a voice: the same segment), which has stored and acknowledged those frames;
 * one that would follow two voices is a mix bus (FR_STREAM_BUS; refused without it with the mix-bus reason), and so is a reader of
 * a bus program's delay line.  Same bits as fr_fill_buffer, in both semantics; it composes with every option above
 * (FR_STREAM_STORE: the tails survive an edit).  With 0 nothing changes: such a plan is refused with "the plan has no fused form
 * ...", a signal delay of a computed value with the reason it has always had, and every other plan is served and refused, with
 * the same reasons, by the same kernels.  "stream" gains "levels" (the levels the stream runs; 1 for every plan that was served
 * before), "short_reads" (ALL the streamed programs' reads below a block of delay lines that programs store, signal reads
 * included -- not only the reads this option admits: with FR_STREAM_LOOPS a loop's reads of its own delay line, the tap behind a
 * loop and a feedback patch's row copies count too) and "dyn_ring_reads" (the signal reads among them, which only this option
 * admits; they count in "dyn_reads" too).  Still refused, each with its reason: a
 * signal delay inside a feedback loop shorter than a block; a feedback patch that delays a computed value by a signal amount (the
 * planner refuses it for fr_fill_buffer too); a bound observed from input rows.
 *
 * FR_STREAM_SWEEP = 0 / 1 (default 0; read strictly from the environment too; acts on top of FR_STREAM_PROGRAMS=1, FR_STREAM_LOOPS=1
 * and FR_STREAM_DYN=1 and does nothing where one of them is missing): block streaming also serves FEEDBACK LOOPS THROUGH A DELAY OF A
 * SIGNAL AMOUNT -- a patch rendered with FR_LOOP_DYN = 1 or 2: a flanger with regeneration, a comb with vibrato, a tape echo
 * x = in + g * Delay(x, base + depth * lfo(t)), with voices or (FR_STREAM_EFFECTS) on a row the host feeds in -- and two neighbours:
 * a Delay by a signal amount inside a feedback loop shorter than a block (a chorus into a comb), and in a feedback patch a signal tap
 * of a delay line that an earlier program stores (a tap behind the loop; a second one makes a mix bus, FR_STREAM_BUS).  The wave that
 * runs such a loop walks the block w frames at a time, w = the proven lower bound of the amount in frames (1..63; at 64 and more the
 * loop reads earlier blocks alone and needs no walk); nobody waits for anybody.  Same bits as fr_fill_buffer, in both semantics; a
 * block that does not continue the previous one is a seek as ever; with FR_STREAM_STORE an edit re-plans and relaunches; FR_RING_KEEP
 * stays inert for such a plan.  With 0 nothing changes: every such plan is refused with the reason it has always had, and every other
 * plan is served and refused, with the same reasons, by the same kernels.  "stream" gains "sweep_programs" (the width of every
 * streamed program, in the order they run; 0: no walk of its own), and "kernel" names the four new kernels (bank_stream_sweep_kernel,
 * bank_stream_sweep_fx_kernel, bank_stream_sweep_store_kernel, bank_stream_sweep_store_fx_kernel) for exactly these plans.  Still
 * refused: an amount whose lower bound the planner cannot prove (FR_ERR_CYCLE, as for fr_fill_buffer), a signal tap of a delay line
 * that a LATER program stores, a bound observed from input rows.
 *
 * FR_STREAM_LEAVES = 0 / 1 (default 0; read strictly from the environment too; does nothing unless FR_STREAM_PROGRAMS=1): block
 * streaming also serves COMPILED VOICES -- voices whose leaves are not the sine partial but share one expression shape: a triangle
 * partial (effects/triangle.fnd), a partial multiplied by a control row, a partial with a phase offset or a divisor; the voices
 * that fr_fill_buffer renders with a kernel generated at run time.  The resident launch does not generate code: it INTERPRETS the
 * leaf, a register program of one instruction per arithmetic primitive (at most 32 instructions over 8 registers), per partial, every
 * operation rounded on its own and the leaves added in the graph's own association -- the same bits as fr_fill_buffer and as the
 * reference, in both semantics.  Such a bank has voices of at least 128 partials and is cut into chunks over the device like a bank
 * of template voices; envelopes, buses, loops, taps, the input history and FR_STREAM_STORE work behind it as behind any bank; next to
 * a bank of another kind or of another leaf shape it needs FR_STREAM_BANKS like any second bank (at most 8 banks).  An input slot
 * other than 0 that a leaf reads -- a gain row, a gate -- is a streamed row: it needs FR_STREAM_INPUTS, counts towards the 8 rows of
 * a block and is listed in "input_slots"; what the leaf reads is what a program's read of that slot at that frame reads.  With 0
 * nothing changes: every such patch is refused with the reason it has always had, and every other plan is served and refused, with
 * the same reasons, by the same kernels.  "stream" gains "leaf_banks" -- per leaf bank in plan order {"ops", "regs", "params",
 * "inputs"}: the leaf's instructions and registers, the parameters per partial, the distinct input slots it reads; [] when the plan
 * has none -- and "kernel" names the two new kernels (bank_stream_leaf_kernel, with FR_STREAM_STORE bank_stream_leaf_store_kernel)
 * for exactly the plans with a leaf bank.  An interpreted leaf costs several times the generated kernel's per partial
 * (profiles/stream_leaves.txt): the option buys the real-time path's features for such patches, not speed.  Still refused, each
 * with its own sentence: compiled voices of 32 or 64 partials; voices that read per-leaf track rows (track voices); a leaf of more
 * than 32 instructions or 8 registers; a compiled bank that is cut over an exchange workspace; a feedback loop through a Delay of a
 * signal amount (FR_STREAM_SWEEP) in a patch with compiled voices.  A plan that has no compiled bank -- while the run-time compiler
 * is still at work, or with FR_JIT=0 -- is answered as it is today: the stream serves the plan in force.
 */
typedef struct fr_option {
    const char *name;              /* e.g. "FR_BANK_SHORT" */
    const char *value;             /* e.g. "0" */
} fr_option;

/* fr_renderer_create plus options.  options == NULL with n_options == 0 is exactly fr_renderer_create. */
fr_status fr_renderer_create_with_options(const fr_config *cfg, const fr_option *options, size_t n_options,
                                          fr_renderer **out);

/* Every per-renderer option as a JSON object: {"FR_BANK_SHORT": {"value": "0", "source": "option"}, ...}; the source is
 * "default", "env" or "option".  The string belongs to the handle and is valid until the next call on it. */
const char *fr_options_json(fr_renderer *r);

/* ---- block streaming with control rows --------------------------------------------------------
 * fr_stream_block (friendship_render.h) with the block's input rows in fr_fill_buffer's own shape: row i -- the floats
 * in_data[in_row_offsets[i] .. in_row_offsets[i + 1]) -- feeds input slot i; fr_stream_block(r, out, n, idx, row, len) is this
 * call with one row.  `out` receives the stream's rows of n_times (1..64) floats each.
 *
 * Statuses and output bits are those of fr_fill_buffer for the same sequence of calls (same slot count, idx and rows) on a
 * renderer whose first call is a seek (with FR_STREAM_STORE=1: on THIS renderer, whatever it has rendered before), although a
 * stream without that option stores no input samples: a short row is padded with its own last
 * value, an empty row that continues with the previous block's last value; a slot that gets no row in a block reads +0.0
 * there; a supplied row must continue its slot's length exactly (FR_ERR_INPUT_HISTORY) and may not be longer than n_times
 * (FR_ERR_INPUT_TOO_LONG); rows at or beyond the input vector count (slots x frames of the largest call so far) are dropped
 * and read +0.0.  Rows of slots that no program reads are checked and otherwise ignored.  A refused block leaves the stream
 * open and everything as it was.  A block that does not continue the previous one is a seek: every input before idx reads
 * 0.0 and every slot starts again.  Plans whose programs read slots other than 0 need FR_STREAM_INPUTS=1 (above). */
fr_status fr_stream_block_rows(fr_renderer *r, float *out, uint64_t n_times, uint64_t idx, const float *in_data,
                               const uint64_t *in_row_offsets, uint32_t n_in_rows);

/* ---- block streaming with a dense matrix: track voices ------------------------------------------
 * fr_stream_block_rows with the block's inputs as fr_fill_buffer_dense takes them: `in` is an [n_in_rows][n_times] row-major
 * matrix.  Its rows below the first declared track slot (fr_set_track_inputs; none declared: all rows) are the block's streamed
 * rows, full length -- row 0 the time row, further rows need FR_STREAM_INPUTS=1 and count towards the 8 rows of a block, exactly
 * as in fr_stream_block_rows.  Its rows from that slot on are the block's TRACKS: per-partial frequency and amplitude rows that
 * the leaves of track voices read at the current frame.  Tracks are read from the block's own matrix and never stored, also under
 * FR_STREAM_STORE=1.
 *
 * Every block equals, bit for bit, what fr_fill_buffer_dense of the same (idx, n_times, in, n_in_rows) returns on a twin renderer
 * with the same call history: a slot at or beyond min(n_in_rows, the input vector count) reads +0.0; a block handed in through
 * fr_stream_block or fr_stream_block_rows brings no matrix and every track reads +0.0 there (not an error); a block that does
 * not continue the previous one is a seek.
 *
 * A stream serves track voices with FR_STREAM_TRACKS = 0 / 1 (default 0; read strictly from the environment too; does nothing
 * unless FR_STREAM_PROGRAMS=1 and FR_STREAM_LEAVES=1): a bank of track voices is then a leaf bank like any other (voices of at
 * least 128 partials, chunks, programs, buses and banks behind it), a track read is one more operand kind of the leaf program (at
 * most 4 distinct track rows per leaf), and the stream stages the rows from the first track slot to the highest slot a voice
 * names -- at most 65536 rows, [rows][64] floats of mapped pinned memory -- which the host fills before it rings the doorbell and
 * the rendering waves read over PCIe one partial ahead of the interpreter.  "stream" gains "tracks": {"first_slot", "rows",
 * "limit"} (rows 0: no leaf reads a track), every entry of "leaf_banks" gains "track_cols", and "kernel" names
 * bank_stream_track_kernel (with FR_STREAM_STORE: bank_stream_track_store_kernel) for exactly the plans that stage tracks.  With
 * 0 nothing changes.  Still refused, each with its own sentence: a track history (FR_TRACK_HISTORY), a program that reads a
 * track, more than 4 track rows per leaf or 65536 per block, and what stays refused for every compiled voice.  On a stream
 * without track voices the call is fr_stream_block_rows with full-length rows.  Cost: profiles/stream_tracks.txt.
 *
 * An optional symbol, as fr_stream_block_rows is. */
fr_status fr_stream_block_dense(fr_renderer *r, float *out, uint64_t n_times, uint64_t idx, const float *in, uint32_t n_in_rows);

#ifdef __cplusplus
}
#endif

#endif /* FRIENDSHIP_RENDER_EXT_H */
