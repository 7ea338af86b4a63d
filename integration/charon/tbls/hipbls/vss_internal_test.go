//go:build hipbls

package hipbls

import (
	"testing"

	promtest "github.com/prometheus/client_golang/prometheus/testutil"
	"github.com/stretchr/testify/require"

	"github.com/obolnetwork/charon/tbls"
)

// commitments are the Feldman commitments to a polynomial whose coefficients the test holds: tbls.Herumi{}'s
// SecretToPublicKey of each coefficient.
func commitments(t *testing.T, coeffs []tbls.PrivateKey) []tbls.PublicKey {
	t.Helper()
	ref := tbls.Herumi{}
	out := make([]tbls.PublicKey, len(coeffs))
	for j, c := range coeffs {
		pk, err := ref.SecretToPublicKey(c)
		require.NoError(t, err)
		out[j] = pk
	}

	return out
}

// TestPublicKeySharesEqualHerumi: a threshold-1 polynomial is its secret alone, so tbls.Herumi{}'s ThresholdSplit with
// threshold 1 gives every share equal to the secret and every pubshare equal to the root key; for threshold 3 the
// pubshares of tbls.Herumi{}'s ThresholdSplit + SecretToPublicKey must satisfy VerifyPubShares against the root key,
// any threshold of them must recover it, and a foreign pubshare must be refused.
func TestPublicKeySharesEqualHerumi(t *testing.T) {
	h, err := New()
	require.NoError(t, err)
	ref := tbls.Herumi{}
	const total, threshold = 5, 3

	items := func(path string) float64 { return promtest.ToFloat64(itemsCounter.WithLabelValues(path)) }
	failed := func(path string) float64 { return promtest.ToFloat64(failedCounter.WithLabelValues(path)) }

	// threshold 1: the public polynomial is the constant root key, at every id
	secret, err := ref.GenerateSecretKey()
	require.NoError(t, err)
	root, err := ref.SecretToPublicKey(secret)
	require.NoError(t, err)
	i0 := items("public_key_share")
	pubs, errs, err := h.PublicKeyShares([][][]tbls.PublicKey{{commitments(t, []tbls.PrivateKey{secret})}}, []int{0, 1, 5, -2})
	require.NoError(t, err)
	require.NoError(t, errs[0])
	require.InDelta(t, 1, items("public_key_share")-i0, 0)
	for _, pk := range pubs[0] {
		require.Equal(t, root, pk)
	}

	// threshold 3: herumi's shares and their public keys
	var groups []map[int]tbls.PublicKey
	var roots []tbls.PublicKey
	var all []map[int]tbls.PublicKey
	for v := 0; v < 4; v++ {
		secret, err := ref.GenerateSecretKey()
		require.NoError(t, err)
		root, err := ref.SecretToPublicKey(secret)
		require.NoError(t, err)
		shares, err := ref.ThresholdSplit(secret, total, threshold)
		require.NoError(t, err)
		pubshares := make(map[int]tbls.PublicKey, total)
		for idx, s := range shares {
			pubshares[idx], err = ref.SecretToPublicKey(s)
			require.NoError(t, err)
		}
		roots = append(roots, root)
		all = append(all, pubshares)
		groups = append(groups, map[int]tbls.PublicKey{1 + v%2: pubshares[1+v%2], 3: pubshares[3], 5: pubshares[5]})
	}
	groups = append(groups, map[int]tbls.PublicKey{}) // empty
	var bad tbls.PublicKey                            // the compression flag is clear
	groups = append(groups, map[int]tbls.PublicKey{1: all[0][1], 2: bad})

	i0, f0 := items("public_key_recover"), failed("public_key_recover")
	keys, errs, err := h.RecoverPublicKeys(groups)
	require.NoError(t, err)
	require.InDelta(t, len(groups), items("public_key_recover")-i0, 0)
	require.InDelta(t, 2, failed("public_key_recover")-f0, 0)
	for v := range roots {
		require.NoError(t, errs[v])
		require.Equal(t, roots[v], keys[v])
	}
	require.Error(t, errs[4])
	require.ErrorContains(t, errs[5], "cannot set compressed public key in Herumi format")

	for v := range roots {
		ok, err := h.VerifyPubShares(roots[v], all[v], threshold)
		require.NoError(t, err)
		require.True(t, ok)
		ok, err = h.VerifyPubShares(roots[(v+1)%4], all[v], threshold)
		require.NoError(t, err)
		require.False(t, ok)
		forged := make(map[int]tbls.PublicKey, total)
		for idx, pk := range all[v] {
			forged[idx] = pk
		}
		forged[4] = all[(v+1)%4][4]
		ok, err = h.VerifyPubShares(roots[v], forged, threshold)
		require.NoError(t, err)
		require.False(t, ok)
	}
}

// TestVerifySecretSharesEqualsHerumi: shares dealt by tbls.Herumi{}'s ThresholdSplit with threshold 1 (the share is the
// secret) pass against the commitment to that secret, and fail against another dealer's or with one bit flipped.
func TestVerifySecretSharesEqualsHerumi(t *testing.T) {
	h, err := New()
	require.NoError(t, err)
	ref := tbls.Herumi{}
	var shares []tbls.PrivateKey
	var coms [][]tbls.PublicKey
	for d := 0; d < 3; d++ {
		secret, err := ref.GenerateSecretKey()
		require.NoError(t, err)
		dealt, err := ref.ThresholdSplit(secret, 4, 1)
		require.NoError(t, err)
		shares = append(shares, dealt[2])
		coms = append(coms, commitments(t, []tbls.PrivateKey{secret}))
	}
	ok, err := h.VerifySecretShares(shares, coms, 2)
	require.NoError(t, err)
	require.Equal(t, []bool{true, true, true}, ok)

	flipped := shares[1]
	flipped[31] ^= 1
	ok, err = h.VerifySecretShares([]tbls.PrivateKey{shares[0], flipped, shares[2]}, coms, 2)
	require.NoError(t, err)
	require.Equal(t, []bool{true, false, true}, ok)

	ok, err = h.VerifySecretShares(shares, [][]tbls.PublicKey{coms[0], coms[2], coms[1]}, 2)
	require.NoError(t, err)
	require.Equal(t, []bool{true, false, false}, ok)

	_, err = h.VerifySecretShares(shares, coms[:2], 2)
	require.Error(t, err)
}
