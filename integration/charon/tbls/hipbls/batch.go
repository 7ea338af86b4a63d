//go:build hipbls

package hipbls

/*
#include "hipbls.h"
*/
import "C"

import (
	"crypto/rand"
	"sort"
	"unsafe"

	"github.com/obolnetwork/charon/app/errors"
	"github.com/obolnetwork/charon/tbls"
)

// The batch extension (tbls.BatchVerifier, patches/0001-tbls-batch-extension.patch): one GPU launch sequence for
// what charon's callers do in loops (core/parsigex/parsigex.go:86-91, core/validatorapi/validatorapi.go:246-283,
// core/sigagg/sigagg.go:138-159).  Every result equals the serial call's for that item: errs[i] is exactly what
// Verify / ThresholdAggregate / VerifyAggregate would return.  A device failure fails the whole call (the error
// return) and is never turned into per-item results.

// BatchVerify verifies n (pk, msg, sig) items in one launch; errs[i] is what Verify returns for item i.
func (HipBLS) BatchVerify(pks []tbls.PublicKey, msgs [][]byte, sigs []tbls.Signature) ([]error, error) {
	n := len(pks)
	if n == 0 {
		return nil, nil
	}
	if len(msgs) != n || len(sigs) != n {
		return nil, errors.New("mismatching lengths")
	}
	flat, offs := flatten(msgs)
	status := make([]int32, n)
	var rc C.int
	path := "batch_verify"
	kidx, keyed, release := lockTable(pks) // held across the call: a reload cannot swap the table under the indices
	if keyed { // keys by resident table index: no per-call decode or subgroup test
		path = "batch_verify_keys"
		rc = C.hipbls_verify_batch_keys((*C.uint32_t)(unsafe.Pointer(&kidx[0])), u8(flat), u64(offs),
			(*C.uint8_t)(unsafe.Pointer(&sigs[0][0])), C.uint64_t(n), i32(status))
	} else {
		rc = C.hipbls_verify_batch((*C.uint8_t)(unsafe.Pointer(&pks[0][0])), u8(flat), u64(offs),
			(*C.uint8_t)(unsafe.Pointer(&sigs[0][0])), C.uint64_t(n), i32(status))
	}
	release()
	if rc != C.HIPBLS_OK {
		return nil, observeFailure(path, n, devErr(rc))
	}
	errs := make([]error, n)
	for i, s := range status {
		errs[i] = verifyErr(s, pks[i][:], sigs[i][:])
	}
	observe(path, errs)

	return errs, nil
}

// BatchVerifyRLC: the same per-item results as BatchVerify, decided by random-linear-combination checks (one
// batch-wide Pippenger check for all-valid batches, windows of 8 otherwise; DESIGN.md 4.6).  msgs are DISTINCT roots,
// msgIdx[i] < len(msgs) names item i's root, and a validator's items should be adjacent.  The seed is fresh from
// crypto/rand on every call: the check is only sound if the signers cannot predict it.
func (HipBLS) BatchVerifyRLC(pks []tbls.PublicKey, sigs []tbls.Signature, msgIdx []uint32, msgs [][]byte) ([]error, error) {
	n := len(pks)
	if n == 0 {
		return nil, nil
	}
	if len(sigs) != n || len(msgIdx) != n {
		return nil, errors.New("mismatching lengths")
	}
	flat, offs := flatten(msgs)
	var seed [32]byte
	if _, err := rand.Read(seed[:]); err != nil {
		return nil, errors.Wrap(err, "rlc seed")
	}
	status := make([]int32, n)
	var rc C.int
	path := "batch_verify_rlc"
	kidx, keyed, release := lockTable(pks) // held across the call, as in BatchVerify
	if keyed { // keys by resident table index
		path = "batch_verify_rlc_keys"
		rc = C.hipbls_batch_verify_rlc_keys((*C.uint32_t)(unsafe.Pointer(&kidx[0])),
			(*C.uint8_t)(unsafe.Pointer(&sigs[0][0])), (*C.uint32_t)(unsafe.Pointer(&msgIdx[0])), C.uint64_t(n), u8(flat),
			u64(offs), C.uint64_t(len(msgs)), u8(seed[:]), i32(status))
	} else {
		rc = C.hipbls_batch_verify_rlc((*C.uint8_t)(unsafe.Pointer(&pks[0][0])),
			(*C.uint8_t)(unsafe.Pointer(&sigs[0][0])), (*C.uint32_t)(unsafe.Pointer(&msgIdx[0])), C.uint64_t(n), u8(flat),
			u64(offs), C.uint64_t(len(msgs)), u8(seed[:]), i32(status))
	}
	release()
	if rc != C.HIPBLS_OK {
		return nil, observeFailure(path, n, devErr(rc))
	}
	errs := make([]error, n)
	for i, s := range status {
		errs[i] = verifyErr(s, pks[i][:], sigs[i][:])
	}
	observe(path, errs)
	observeRLC()

	return errs, nil
}

// groupsFlat lays out ThresholdAggregate groups for the C-ABI: signatures, int64 ids (map keys, no truncation) and
// group offsets.  Map iteration order is irrelevant to the result (Lagrange at 0 is symmetric).
func groupsFlat(groups []map[int]tbls.Signature) ([]byte, []int64, []uint64) {
	var sigs []byte
	var ids []int64
	offs := []uint64{0}
	for _, g := range groups {
		for idx, s := range g {
			sigs = append(sigs, s[:]...)
			ids = append(ids, int64(idx))
		}
		offs = append(offs, uint64(len(ids)))
	}

	return sigs, ids, offs
}

// aggErr maps an aggregation status onto herumi's error text (tbls/herumi.go:244-283).
func aggErr(s int32) error {
	switch C.int32_t(s) {
	case C.HIPBLS_OK:
		return nil
	case C.HIPBLS_ERR_SIGNATURE:
		return errors.New("cannot unmarshal signature into Herumi signature")
	default: // empty group, id 0 (mod r), duplicate id
		return errors.New("cannot combine signatures")
	}
}

// BatchThresholdAggregate: one output signature (or error) per group.
func (HipBLS) BatchThresholdAggregate(groups []map[int]tbls.Signature) ([]tbls.Signature, []error, error) {
	if len(groups) == 0 {
		return nil, nil, nil
	}
	sigs, ids, offs := groupsFlat(groups)
	out := make([]tbls.Signature, len(groups))
	status := make([]int32, len(groups))
	rc := C.hipbls_threshold_aggregate_batch(u8(sigs), i64(ids), u64(offs), C.uint64_t(len(groups)),
		(*C.uint8_t)(unsafe.Pointer(&out[0][0])), i32(status))
	if rc != C.HIPBLS_OK {
		return nil, nil, observeFailure("threshold_aggregate", len(groups), devErr(rc))
	}
	errs := make([]error, len(groups))
	for g, s := range status {
		errs[g] = aggErr(s)
	}
	observe("threshold_aggregate", errs)

	return out, errs, nil
}

// BatchVerifyAggregate: one FastAggregateVerify per (keys, sig, msg) group in one launch (cluster.Lock
// VerifySignatures over every lock and registration, cluster/lock.go:144-274).
func (h HipBLS) BatchVerifyAggregate(keys [][]tbls.PublicKey, sigs []tbls.Signature, msgs [][]byte) ([]error, error) {
	g := len(keys)
	if g == 0 {
		return nil, nil
	}
	if len(sigs) != g || len(msgs) != g {
		return nil, errors.New("mismatching lengths")
	}
	var flatKeys []byte
	var allKeys []tbls.PublicKey
	koffs := make([]uint64, g+1)
	for i, ks := range keys {
		for _, k := range ks {
			flatKeys = append(flatKeys, k[:]...)
		}
		allKeys = append(allKeys, ks...)
		koffs[i+1] = uint64(len(flatKeys) / 48)
	}
	flat, moffs := flatten(msgs)
	status := make([]int32, g)
	var rc C.int
	path := "batch_verify_aggregate"
	kidx, keyed, release := lockTable(allKeys) // held across the call, as in BatchVerify
	if keyed && len(allKeys) > 0 { // every key of every group by resident table index: no decode, H(m) from the cache
		path = "batch_verify_aggregate_keys"
		rc = C.hipbls_verify_aggregate_batch_keys((*C.uint32_t)(unsafe.Pointer(&kidx[0])), u64(koffs), C.uint64_t(g),
			(*C.uint8_t)(unsafe.Pointer(&sigs[0][0])), u8(flat), u64(moffs), i32(status))
	} else {
		rc = C.hipbls_verify_aggregate_batch(u8(flatKeys), u64(koffs), C.uint64_t(g),
			(*C.uint8_t)(unsafe.Pointer(&sigs[0][0])), u8(flat), u64(moffs), i32(status))
	}
	release()
	if rc != C.HIPBLS_OK {
		return nil, observeFailure(path, g, devErr(rc))
	}
	errs := make([]error, g)
	for i, s := range status {
		switch C.int32_t(s) {
		case C.HIPBLS_OK:
		case C.HIPBLS_ERR_SIGNATURE:
			errs[i] = deserErr(C.HIPBLS_ERR_SIGNATURE, nil, sigs[i][:])
		case C.HIPBLS_ERR_PUBKEY: // name the key as VerifyAggregate does
			errs[i] = h.VerifyAggregate(keys[i], sigs[i], msgs[i])
		default:
			errs[i] = errors.New("signature verification failed")
		}
	}
	observe(path, errs)

	return errs, nil
}

// BatchThresholdAggregateVerify: core/sigagg in one call (sigagg.go:138-159).  For each validator g: the aggregate
// of its partials (or the aggregation error) and the error Verify(dvPks[g], msgs[g], aggregate) would return (the
// aggregation's error when it failed).  Same results as BatchThresholdAggregate + BatchVerify; the root key decode
// and H(m) run beside the aggregation and the aggregate is not decompressed again (DESIGN.md 4.9).
//
// With sigaggByKeys set and every root key in the resident table (app.go loads them beside the pubshares) the call
// names them by index and passes the DISTINCT roots: no key decode or subgroup test, each root read from the H(m) cache
// that the RLC BatchVerify of its partials filled, or hashed once (DESIGN.md 4.9.1).  Otherwise the wire-format call.
func (HipBLS) BatchThresholdAggregateVerify(groups []map[int]tbls.Signature, dvPks []tbls.PublicKey,
	msgs [][]byte,
) ([]tbls.Signature, []error, []error, error) {
	n := len(groups)
	if n == 0 {
		return nil, nil, nil, nil
	}
	if len(dvPks) != n || len(msgs) != n {
		return nil, nil, nil, errors.New("mismatching lengths")
	}
	sigs, ids, offs := groupsFlat(groups)
	out := make([]tbls.Signature, n)
	ast := make([]int32, n)
	vst := make([]int32, n)
	var rc C.int
	path := "fused_sigagg"
	var kidx []uint32
	keyed, release := false, func() {}
	if sigaggByKeys {
		kidx, keyed, release = lockTable(dvPks) // held across the call, as in BatchVerify
	}
	if keyed {
		path = "batch_threshold_aggregate_verify_keys"
		roots, midx := distinctRoots(msgs)
		flat, moffs := flatten(roots)
		rc = C.hipbls_threshold_aggregate_verify_batch_keys(u8(sigs), i64(ids), u64(offs), C.uint64_t(n),
			(*C.uint32_t)(unsafe.Pointer(&kidx[0])), (*C.uint32_t)(unsafe.Pointer(&midx[0])), u8(flat), u64(moffs),
			C.uint64_t(len(roots)), (*C.uint8_t)(unsafe.Pointer(&out[0][0])), i32(ast), i32(vst))
	} else {
		flat, moffs := flatten(msgs)
		rc = C.hipbls_threshold_aggregate_verify_batch(u8(sigs), i64(ids), u64(offs), C.uint64_t(n),
			(*C.uint8_t)(unsafe.Pointer(&dvPks[0][0])), u8(flat), u64(moffs), (*C.uint8_t)(unsafe.Pointer(&out[0][0])),
			i32(ast), i32(vst))
	}
	release()
	if rc != C.HIPBLS_OK {
		return nil, nil, nil, observeFailure(path, n, devErr(rc))
	}
	aggErrs := make([]error, n)
	verErrs := make([]error, n)
	for g := range groups {
		aggErrs[g] = aggErr(ast[g])
		if aggErrs[g] != nil {
			verErrs[g] = aggErrs[g]
		} else {
			verErrs[g] = verifyErr(vst[g], dvPks[g][:], out[g][:])
		}
	}
	observe(path, verErrs)

	return out, aggErrs, verErrs, nil
}

// sigaggByKeys: BatchThresholdAggregateVerify takes the keyed call when every root key is resident.  Results are the
// same either way, so the default rests on the measured times (DESIGN.md 4.9.1, profiles/r08): the keyed call with a
// warm cache is 1.0 ms faster on a lone 7-of-10 duty (9.1 against 10.1 ms p50), but 2-3 % slower on 10,000 validators
// with 10,000 distinct roots from two threads (its cache lookups run on the host under the context lock, and the
// hashes they save were hidden beside the partials' scaling anyway), so the wire-format call stays the default.
var sigaggByKeys = false

// distinctRoots dedupes the groups' messages (an attester duty's validators share one root per committee) into the
// distinct-message table of the keyed call: roots in first-use order and each group's index into them.
func distinctRoots(msgs [][]byte) ([][]byte, []uint32) {
	pos := make(map[string]uint32, len(msgs))
	var roots [][]byte
	midx := make([]uint32, len(msgs))
	for g, m := range msgs {
		j, ok := pos[string(m)]
		if !ok {
			j = uint32(len(roots))
			pos[string(m)] = j
			roots = append(roots, m)
		}
		midx[g] = j
	}

	return roots, midx
}

// Dealt is one validator's result of BatchThresholdSplit: the shares f(i) and their public keys, i = 1..total, and the
// root public key [f(0)] g1.
type Dealt struct {
	Shares    map[int]tbls.PrivateKey
	PubKey    tbls.PublicKey
	PubShares map[int]tbls.PublicKey
}

// BatchThresholdSplit deals every secret in one call: what dkg/keycast.go:156-179 does per validator
// (SecretToPublicKey of the root, ThresholdSplit, SecretToPublicKey of each share), on kernels whose instruction stream
// and memory addresses do not depend on the secrets (hipbls_threshold_split_batch_ct).  The polynomial tails come from
// crypto/rand as ThresholdSplit's do.  errs[v] is what the serial calls return for validator v.
func (h HipBLS) BatchThresholdSplit(secrets []tbls.PrivateKey, total, threshold uint) ([]Dealt, []error, error) {
	n := len(secrets)
	if n == 0 {
		return nil, nil, nil
	}
	flat := make([]byte, 0, 32*n)
	poly := make([]byte, 0, 32*n*int(threshold))
	for _, s := range secrets {
		flat = append(flat, s[:]...)
		for i := 1; i < int(threshold); i++ {
			k, err := h.GenerateSecretKey()
			if err != nil {
				return nil, nil, err
			}
			poly = append(poly, k[:]...)
		}
	}
	row := int(total) + 1
	shares := make([]byte, 32*n*int(total))
	pubs := make([]byte, 48*n*row)
	status := make([]int32, n)
	pubStatus := make([]int32, n*row)
	if rc := C.hipbls_threshold_split_batch_ct(u8(flat), u8(poly), C.uint64_t(n), C.uint32_t(total),
		C.uint32_t(threshold), u8(shares), i32(status), u8(pubs), i32(pubStatus)); rc != C.HIPBLS_OK {
		return nil, nil, observeFailure("threshold_split", n, devErr(rc))
	}
	out := make([]Dealt, n)
	errs := make([]error, n)
	for v := range secrets {
		if status[v] != C.HIPBLS_OK {
			errs[v] = errors.New("cannot unmarshal bytes into Herumi secret key")
			continue
		}
		d := Dealt{Shares: make(map[int]tbls.PrivateKey, total), PubShares: make(map[int]tbls.PublicKey, total)}
		for k := 0; k < row; k++ {
			if pubStatus[v*row+k] != C.HIPBLS_OK { // a zero scalar: GetSafePublicKey fails (herumi.go:74)
				errs[v] = errors.New("cannot obtain public key from secret")
				break
			}
			var pk tbls.PublicKey
			copy(pk[:], pubs[48*(v*row+k):])
			if k == 0 {
				d.PubKey = pk
				continue
			}
			var sk tbls.PrivateKey
			copy(sk[:], shares[32*(v*int(total)+k-1):])
			d.Shares[k] = sk
			d.PubShares[k] = pk
		}
		if errs[v] == nil {
			out[v] = d
		}
	}
	observe("threshold_split", errs)

	return out, errs, nil
}

// BatchRecoverSecret recovers one secret per group and its public key in one call: what cmd/combine/combine.go:106-119
// does per validator (RecoverSecret, SecretToPublicKey), secret-independent (hipbls_recover_secret_batch_ct).  errs[g]
// is what the serial calls return for group g.
func (HipBLS) BatchRecoverSecret(groups []map[int]tbls.PrivateKey) ([]tbls.PrivateKey, []tbls.PublicKey, []error, error) {
	n := len(groups)
	if n == 0 {
		return nil, nil, nil, nil
	}
	var flat []byte
	var ids []int64
	offs := []uint64{0}
	for _, g := range groups {
		for idx, k := range g {
			flat = append(flat, k[:]...)
			ids = append(ids, int64(idx))
		}
		offs = append(offs, uint64(len(ids)))
	}
	secrets := make([]tbls.PrivateKey, n)
	pks := make([]tbls.PublicKey, n)
	status := make([]int32, n)
	pkStatus := make([]int32, n)
	if rc := C.hipbls_recover_secret_batch_ct(u8(flat), i64(ids), u64(offs), C.uint64_t(n),
		(*C.uint8_t)(unsafe.Pointer(&secrets[0][0])), i32(status), (*C.uint8_t)(unsafe.Pointer(&pks[0][0])),
		i32(pkStatus)); rc != C.HIPBLS_OK {
		return nil, nil, nil, observeFailure("recover_secret", n, devErr(rc))
	}
	errs := make([]error, n)
	for g := range groups {
		switch {
		case status[g] == C.HIPBLS_ERR_SECRET:
			errs[g] = errors.New("cannot unmarshal key with into Herumi secret key")
		case status[g] != C.HIPBLS_OK:
			errs[g] = errors.New("cannot recover full private key from partial keys")
		case pkStatus[g] != C.HIPBLS_OK:
			errs[g] = errors.New("cannot obtain public key from secret")
		}
	}
	observe("recover_secret", errs)

	return secrets, pks, errs, nil
}

// PublicKeyShares evaluates every validator's public polynomial at every id in one call (herumi's blsPublicKeyShare;
// hipbls_public_key_share_batch).  commitments[v][d][j] is dealer d's Feldman commitment to coefficient j of validator
// v's polynomial; the dealers' polynomials are added, so a joint dealing (FROST) needs no host arithmetic.  ids are the
// cluster's operator indices, shared by every validator; id 0 gives the validator's group public key.  out[v][i] is
// the key at ids[i]; errs[v] is set when a commitment of v does not deserialize.  Not a method of tbls.Implementation.
func (HipBLS) PublicKeyShares(commitments [][][]tbls.PublicKey, ids []int) ([][]tbls.PublicKey, []error, error) {
	n := len(commitments)
	if n == 0 {
		return nil, nil, nil
	}
	dealers := len(commitments[0])
	if dealers == 0 || len(commitments[0][0]) == 0 || len(ids) == 0 {
		return nil, nil, errors.New("public key shares need a dealer, a commitment and an id")
	}
	threshold := len(commitments[0][0])
	flat := make([]byte, 0, 48*n*dealers*threshold)
	for _, val := range commitments {
		if len(val) != dealers {
			return nil, nil, errors.New("every validator has the same number of dealers")
		}
		for _, poly := range val {
			if len(poly) != threshold {
				return nil, nil, errors.New("every polynomial has threshold commitments")
			}
			for _, c := range poly {
				flat = append(flat, c[:]...)
			}
		}
	}
	xs := make([]int64, len(ids))
	for i, id := range ids {
		xs[i] = int64(id)
	}
	pubs := make([]byte, 48*n*len(ids))
	status := make([]int32, n)
	if rc := C.hipbls_public_key_share_batch(u8(flat), C.uint64_t(n), C.uint32_t(dealers), C.uint32_t(threshold),
		i64(xs), C.uint32_t(len(ids)), u8(pubs), i32(status)); rc != C.HIPBLS_OK {
		return nil, nil, observeFailure("public_key_share", n, devErr(rc))
	}
	out := make([][]tbls.PublicKey, n)
	errs := make([]error, n)
	for v := range commitments {
		if status[v] != C.HIPBLS_OK {
			errs[v] = errors.New("cannot set compressed public key in Herumi format")
			continue
		}
		out[v] = make([]tbls.PublicKey, len(ids))
		for i := range ids {
			copy(out[v][i][:], pubs[48*(v*len(ids)+i):])
		}
	}
	observe("public_key_share", errs)

	return out, errs, nil
}

// RecoverPublicKeys recovers one public key per group of pubshares in one call (herumi's blsPublicKeyRecover: Lagrange
// at 0 over G1; hipbls_public_key_recover_batch).  errs[g] is set for an empty group, a share index 0 or a pubshare that
// does not deserialize.  Not a method of tbls.Implementation.
func (HipBLS) RecoverPublicKeys(groups []map[int]tbls.PublicKey) ([]tbls.PublicKey, []error, error) {
	n := len(groups)
	if n == 0 {
		return nil, nil, nil
	}
	var flat []byte
	var ids []int64
	offs := []uint64{0}
	for _, g := range groups {
		for idx, k := range g {
			flat = append(flat, k[:]...)
			ids = append(ids, int64(idx))
		}
		offs = append(offs, uint64(len(ids)))
	}
	pks := make([]tbls.PublicKey, n)
	status := make([]int32, n)
	if rc := C.hipbls_public_key_recover_batch(u8(flat), i64(ids), u64(offs), C.uint64_t(n),
		(*C.uint8_t)(unsafe.Pointer(&pks[0][0])), i32(status)); rc != C.HIPBLS_OK {
		return nil, nil, observeFailure("public_key_recover", n, devErr(rc))
	}
	errs := make([]error, n)
	for g := range groups {
		switch {
		case status[g] == C.HIPBLS_ERR_PUBKEY:
			errs[g] = errors.New("cannot set compressed public key in Herumi format")
		case status[g] != C.HIPBLS_OK:
			errs[g] = errors.New("cannot recover public key from public key shares")
		}
	}
	observe("public_key_recover", errs)

	return pks, errs, nil
}

// VerifySecretShares is the Feldman check of received shares: shares[d] is what dealer d sent this node (operator index
// myID) and commitments[d] that dealer's commitments to its polynomial.  ok[d] says whether [shares[d]] g1 equals the
// dealer's public polynomial at myID.  Both sides are public values; [share] g1 comes from the secret-independent
// kernel (hipbls_secret_to_public_key_batch_ct).
func (h HipBLS) VerifySecretShares(shares []tbls.PrivateKey, commitments [][]tbls.PublicKey, myID int) ([]bool, error) {
	n := len(shares)
	if n != len(commitments) {
		return nil, errors.New("one commitment list per share")
	}
	if n == 0 {
		return nil, nil
	}
	flat := make([]byte, 0, 32*n)
	polys := make([][][]tbls.PublicKey, n)
	for d, s := range shares {
		flat = append(flat, s[:]...)
		polys[d] = [][]tbls.PublicKey{commitments[d]}
	}
	pks := make([]tbls.PublicKey, n)
	status := make([]int32, n)
	if rc := C.hipbls_secret_to_public_key_batch_ct(u8(flat), C.uint64_t(n), (*C.uint8_t)(unsafe.Pointer(&pks[0][0])),
		i32(status)); rc != C.HIPBLS_OK {
		return nil, observeFailure("public_key_share", n, devErr(rc))
	}
	want, errs, err := h.PublicKeyShares(polys, []int{myID})
	if err != nil {
		return nil, err
	}
	ok := make([]bool, n)
	for d := range shares {
		ok[d] = status[d] == C.HIPBLS_OK && errs[d] == nil && pks[d] == want[d][0]
	}

	return ok, nil
}

// VerifyPubShares says whether every pubshare lies on the one polynomial of degree threshold-1 whose value at 0 is
// pubkey, in one RecoverPublicKeys call: the threshold pubshares with the smallest indices must recover pubkey, and for
// every further index k the same pubshares at indices shifted to idx-k must recover pubshares[k] (Lagrange at k over
// x_j is Lagrange at 0 over x_j-k).
func (h HipBLS) VerifyPubShares(pubkey tbls.PublicKey, pubshares map[int]tbls.PublicKey, threshold int) (bool, error) {
	if threshold < 1 || len(pubshares) < threshold {
		return false, nil
	}
	idxs := make([]int, 0, len(pubshares))
	for idx := range pubshares {
		idxs = append(idxs, idx)
	}
	sort.Ints(idxs)
	base, rest := idxs[:threshold], idxs[threshold:]
	groups := make([]map[int]tbls.PublicKey, 0, 1+len(rest))
	want := make([]tbls.PublicKey, 0, 1+len(rest))
	for _, k := range append([]int{0}, rest...) {
		g := make(map[int]tbls.PublicKey, threshold)
		for _, idx := range base {
			g[idx-k] = pubshares[idx]
		}
		groups = append(groups, g)
		if len(want) == 0 {
			want = append(want, pubkey)
		} else {
			want = append(want, pubshares[k])
		}
	}
	got, errs, err := h.RecoverPublicKeys(groups)
	if err != nil {
		return false, err
	}
	for g := range groups {
		if errs[g] != nil || got[g] != want[g] {
			return false, nil
		}
	}

	return true, nil
}

// DealtCommitted is one validator's result of DealWithCommitments: the shares f(i), i = 1..total, and the Feldman
// commitments [a_j] g1 to the coefficients of f, j = 0..threshold-1 (Commitments[0] is the dealer's public key for
// this validator).
type DealtCommitted struct {
	Shares      map[int]tbls.PrivateKey
	Commitments []tbls.PublicKey
}

// DealWithCommitments is a dealer's round 1 of a joint-Feldman dealing for every validator in one call: what
// dkg/frost.go:117-149 does validator by validator in kryptology (the shares for every operator and the commitments to
// broadcast), on kernels whose instruction stream and memory addresses do not depend on the secrets
// (hipbls_deal_commit_batch_ct).  The polynomial tails come from crypto/rand as ThresholdSplit's do.  errs[v] is set
// when the secret of validator v is not a scalar.  Not a method of tbls.Implementation.
func (h HipBLS) DealWithCommitments(secrets []tbls.PrivateKey, total, threshold uint) ([]DealtCommitted, []error, error) {
	n := len(secrets)
	if n == 0 {
		return nil, nil, nil
	}
	flat := make([]byte, 0, 32*n)
	poly := make([]byte, 0, 32*n*int(threshold))
	for _, s := range secrets {
		flat = append(flat, s[:]...)
		for i := 1; i < int(threshold); i++ {
			k, err := h.GenerateSecretKey()
			if err != nil {
				return nil, nil, err
			}
			poly = append(poly, k[:]...)
		}
	}
	shares := make([]byte, 32*n*int(total))
	coms := make([]byte, 48*n*int(threshold))
	status := make([]int32, n)
	comStatus := make([]int32, n*int(threshold))
	if rc := C.hipbls_deal_commit_batch_ct(u8(flat), u8(poly), C.uint64_t(n), C.uint32_t(total), C.uint32_t(threshold),
		u8(shares), i32(status), u8(coms), i32(comStatus)); rc != C.HIPBLS_OK {
		return nil, nil, observeFailure("deal_commit", n, devErr(rc))
	}
	out := make([]DealtCommitted, n)
	errs := make([]error, n)
	for v := range secrets {
		if status[v] != C.HIPBLS_OK {
			errs[v] = errors.New("cannot unmarshal bytes into Herumi secret key")
			continue
		}
		d := DealtCommitted{Shares: make(map[int]tbls.PrivateKey, total), Commitments: make([]tbls.PublicKey, threshold)}
		for k := 1; k <= int(total); k++ {
			var sk tbls.PrivateKey
			copy(sk[:], shares[32*(v*int(total)+k-1):])
			d.Shares[k] = sk
		}
		for j := range d.Commitments {
			copy(d.Commitments[j][:], coms[48*(v*int(threshold)+j):])
		}
		out[v] = d
	}
	observe("deal_commit", errs)

	return out, errs, nil
}

// VerifySecretSharesBatch is a receiver's round 2 check for every validator in one call (dkg/frost.go:198-248;
// hipbls_verify_secret_shares_batch_ct): shares[v][d] is what dealer d sent this node (operator index myID) for
// validator v, commitments[v][d] that dealer's commitments.  errs[v][d] is nil when [shares[v][d]] g1 equals the
// dealer's public polynomial at myID; the comparison is made on the device and only the verdicts come back.  Not a
// method of tbls.Implementation.
func (HipBLS) VerifySecretSharesBatch(shares [][]tbls.PrivateKey, commitments [][][]tbls.PublicKey, myID int) ([][]error, error) {
	n := len(shares)
	if n != len(commitments) {
		return nil, errors.New("one commitment list per share")
	}
	if n == 0 {
		return nil, nil
	}
	dealers := len(shares[0])
	if dealers == 0 || len(commitments[0]) != dealers || len(commitments[0][0]) == 0 {
		return nil, errors.New("share checks need a dealer and a commitment")
	}
	threshold := len(commitments[0][0])
	flat := make([]byte, 0, 32*n*dealers)
	coms := make([]byte, 0, 48*n*dealers*threshold)
	for v := range shares {
		if len(shares[v]) != dealers || len(commitments[v]) != dealers {
			return nil, errors.New("every validator has the same number of dealers")
		}
		for d := range shares[v] {
			flat = append(flat, shares[v][d][:]...)
			if len(commitments[v][d]) != threshold {
				return nil, errors.New("every polynomial has threshold commitments")
			}
			for _, c := range commitments[v][d] {
				coms = append(coms, c[:]...)
			}
		}
	}
	status := make([]int32, n*dealers)
	if rc := C.hipbls_verify_secret_shares_batch_ct(u8(flat), u8(coms), C.uint64_t(n), C.uint32_t(dealers),
		C.uint32_t(threshold), C.int64_t(myID), i32(status)); rc != C.HIPBLS_OK {
		return nil, observeFailure("verify_secret_shares", n*dealers, devErr(rc))
	}
	out := make([][]error, n)
	all := make([]error, 0, n*dealers)
	for v := range shares {
		out[v] = make([]error, dealers)
		for d := range out[v] {
			switch status[v*dealers+d] {
			case C.HIPBLS_OK:
			case C.HIPBLS_ERR_PUBKEY:
				out[v][d] = errors.New("cannot set compressed public key in Herumi format")
			case C.HIPBLS_ERR_SECRET:
				out[v][d] = errors.New("cannot unmarshal bytes into Herumi secret key")
			default:
				out[v][d] = errors.New("secret share does not match the dealer's commitments")
			}
			all = append(all, out[v][d])
		}
	}
	observe("verify_secret_shares", all)

	return out, nil
}

// CombineShares is the last step of a joint dealing for every validator in one call
// (hipbls_combine_shares_batch_ct): this node's final share of validator v is the sum of shares[v][d] over the dealers
// with include[v][d] (a nil include takes every dealer), and its pubshare follows from it, with no secret passing
// through host integers.  errs[v] is set when no dealer is included, an included share is not a scalar, or the sum is
// zero (a secret without a public key).  Not a method of tbls.Implementation.
func (HipBLS) CombineShares(shares [][]tbls.PrivateKey, include [][]bool) ([]tbls.PrivateKey, []tbls.PublicKey, []error, error) {
	n := len(shares)
	if n == 0 {
		return nil, nil, nil, nil
	}
	dealers := len(shares[0])
	if dealers == 0 || (include != nil && len(include) != n) {
		return nil, nil, nil, errors.New("combining shares needs a dealer and one include flag per share")
	}
	flat := make([]byte, 0, 32*n*dealers)
	var mask []byte
	for v := range shares {
		if len(shares[v]) != dealers || (include != nil && len(include[v]) != dealers) {
			return nil, nil, nil, errors.New("every validator has the same number of dealers")
		}
		for d := range shares[v] {
			flat = append(flat, shares[v][d][:]...)
			if include != nil {
				var b byte
				if include[v][d] {
					b = 1
				}
				mask = append(mask, b)
			}
		}
	}
	sums := make([]tbls.PrivateKey, n)
	pubs := make([]tbls.PublicKey, n)
	status := make([]int32, n)
	pubStatus := make([]int32, n)
	if rc := C.hipbls_combine_shares_batch_ct(u8(flat), u8(mask), C.uint64_t(n), C.uint32_t(dealers),
		(*C.uint8_t)(unsafe.Pointer(&sums[0][0])), i32(status), (*C.uint8_t)(unsafe.Pointer(&pubs[0][0])),
		i32(pubStatus)); rc != C.HIPBLS_OK {
		return nil, nil, nil, observeFailure("combine_shares", n, devErr(rc))
	}
	errs := make([]error, n)
	for v := range shares {
		switch {
		case status[v] == C.HIPBLS_ERR_SECRET:
			errs[v] = errors.New("cannot unmarshal bytes into Herumi secret key")
		case status[v] != C.HIPBLS_OK:
			errs[v] = errors.New("no qualified dealer to combine shares from")
		case pubStatus[v] != C.HIPBLS_OK:
			errs[v] = errors.New("cannot obtain public key from secret")
		}
	}
	observe("combine_shares", errs)

	return sums, pubs, errs, nil
}
